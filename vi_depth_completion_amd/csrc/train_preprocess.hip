// Training-batch pre-processing on the device (second half): the per-frame arithmetic of the reference's
// ScanNetSmallFramesDataset.__getitem__ (dataset.py:95-247) and NYUDataset.__getitem__ (dataset.py:381-438) -- byte images to the
// loaders' float tensors, the sparse map of the pixel-coordinate tracks, the random sparse sample of the ground truth
// (torch.nonzero + permutation + scatter) and NYU's depth range rule -- so that a trainer stepping at several hundred frames per
// second is not fed by a PIL / numpy DataLoader.  Everything is bit-identical to the host sequence it replaces.
#include "common.h"
#include <cstdint>

namespace {

constexpr int TPB = 256;

// ---- (a) uint8 HWC -> float CHW ---------------------------------------------------------------------------------------------------
// Every operation rounded once, in the reference's order (nothing contracted).
__device__ inline float decode_byte(int x, int mode) {
    const float v = (float)x;
    if (mode <= 1) {
        const float t = __fdiv_rn(v, 255.0f);                       // ToTensor
        return mode == 0 ? t : __fadd_rn(-t, 0.5f);                 // Z = -ToTensor(orient) + 0.5
    }
    const float t = __fsub_rn(1.0f, __fdiv_rn(v, 127.5f));          // 1 - x / 127.5
    return mode == 2 ? t : __fadd_rn(-t, 0.5f);
}

// A byte has 256 values: each workgroup evaluates the expression once per value into LDS and the pixels look it up (the same bits as
// evaluating it per pixel, without an IEEE division per element in a kernel that should run at memory speed).
__device__ inline void fill_lut(float* lut, int mode) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = decode_byte(i, mode);
    __syncthreads();
}

// 16 consecutive pixels per thread: C 16-byte loads, 4 16-byte stores per channel plane.  Needs HW % 16 == 0 and 16-byte-aligned bases.
template <int C>
__global__ void __launch_bounds__(TPB)
u8_decode_vec_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int HW, int mode) {
    __shared__ float lut[256];
    fill_lut(lut, mode);
    const int b = blockIdx.y;
    const long long p0 = ((long long)blockIdx.x * TPB + threadIdx.x) * 16;
    if (p0 >= HW) return;
    const uint4* s = reinterpret_cast<const uint4*>(src + ((size_t)b * HW + p0) * C);
    unsigned w[4 * C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const uint4 q = s[k];
        w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float4* d = reinterpret_cast<float4*>(dst + ((size_t)b * C + c) * HW + p0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = (4 * j + e) * C + c;                  // byte index inside the thread's 16 * C bytes
                o[e] = lut[(w[k >> 2] >> (8 * (k & 3))) & 255u];
            }
            d[j] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// One output element per thread: any size, any alignment.
__global__ void __launch_bounds__(TPB)
u8_decode_scalar_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int HW, int C, int mode) {
    __shared__ float lut[256];
    fill_lut(lut, mode);
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;      // (c, p) of image b
    if (i >= (long long)C * HW) return;
    const int c = (int)(i / HW);
    const long long p = i - (long long)c * HW;
    dst[(size_t)b * C * HW + i] = lut[src[((size_t)b * HW + p) * C + c]];
}

// ---- (b) pixel-coordinate tracks -> sparse map ------------------------------------------------------------------------------------
// The reference's loop is sequential and a later track overwrites an earlier one: the winner of a pixel is its highest track index.
// Phase 1 clears the winner map, phase 2 gives every track a lane and takes the maximum atomically (integer max: order-free, so
// the result is deterministic), phase 3 writes every pixel of the map: the winner's value, or 0.
__global__ void __launch_bounds__(TPB)
tracks_clear_kernel(int32_t* __restrict__ winner, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) winner[i] = -1;
}

__global__ void __launch_bounds__(TPB)
tracks_vote_kernel(const double* __restrict__ tracks, const int32_t* __restrict__ offsets, int n_tracks, int B, double divisor,
                   int32_t* __restrict__ winner, int H, int W) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n_tracks) return;
    int b = -1;
    for (int k = 0; k < B; ++k)
        if (i >= offsets[k] && i < offsets[k + 1]) b = k;
    if (b < 0) return;                                              // a row no image owns
    const double qx = __ddiv_rn(tracks[4 * (size_t)i + 1], divisor), qy = __ddiv_rn(tracks[4 * (size_t)i + 2], divisor);
    // astype(np.int32) / int() of a NaN or of a value beyond int32 is no pixel
    if (!(qx > -2147483649.0 && qx < 2147483648.0 && qy > -2147483649.0 && qy < 2147483648.0)) return;
    const int col = (int)qx, row = (int)qy;                         // truncation toward zero: -0.5 is pixel 0
    if (row >= 0 && row < H && col >= 0 && col < W) atomicMax(&winner[((size_t)b * H + row) * W + col], i);
}

__global__ void __launch_bounds__(TPB)
tracks_write_kernel(const double* __restrict__ tracks, const int32_t* __restrict__ winner, const float* __restrict__ gt,
                    float* __restrict__ depth, long long n, int n_tracks) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int w = winner[i];
    float v = 0.f;
    if (w >= 0 && w < n_tracks) v = gt ? gt[i] : (float)tracks[4 * (size_t)w + 3];
    depth[i] = v;
}

// ---- (c) torch.nonzero of a float map, per image ----------------------------------------------------------------------------------
// A workgroup owns NZ_CHUNK consecutive elements of one image; each of its four waves owns 256 of them and walks them 64 at a time, so
// a wave-wide ballot is a bit mask in index order: its population count is the count, the bits below a lane are the lane's rank.
// Launch 1 writes one count per chunk.  Launch 2 sums the counts of the chunks in front of its own (a few dozen numbers, read by
// every workgroup: no workgroup waits for another), repeats the ballots and writes the indices.
constexpr int NZ_CHUNK = VIDC_NONZERO_CHUNK, NZ_WAVES = TPB / 64, NZ_ITERS = NZ_CHUNK / TPB;
static_assert(NZ_WAVES * NZ_ITERS * 64 == NZ_CHUNK, "a chunk is whole wave passes");

__device__ inline unsigned long long nz_ballot(const float* __restrict__ v, int HW, int i) {
    // torch.nonzero's `!= 0` on the bits (whatever the wave's denormal mode): NaN and denormals count, -0.0 does not
    return __ballot(i < HW && (__float_as_uint(v[i]) << 1) != 0u);
}

__global__ void __launch_bounds__(TPB)
nonzero_count_kernel(const float* __restrict__ v, int HW, int nchunks, int32_t* __restrict__ chunk_count) {
    __shared__ int wsum[NZ_WAVES];
    const int b = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* vb = v + (size_t)b * HW;
    const int base = chunk * NZ_CHUNK + wave * (NZ_ITERS * 64);
    int n = 0;
#pragma unroll
    for (int it = 0; it < NZ_ITERS; ++it) n += __popcll(nz_ballot(vb, HW, base + it * 64 + lane));
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < NZ_WAVES; ++k) s += wsum[k];
        chunk_count[(size_t)b * nchunks + chunk] = s;
    }
}

__global__ void __launch_bounds__(TPB)
nonzero_scatter_kernel(const float* __restrict__ v, int HW, int nchunks, const int32_t* __restrict__ chunk_count,
                       int32_t* __restrict__ count, int32_t* __restrict__ index) {
    __shared__ int before[TPB], total[TPB], wsum[NZ_WAVES];
    const int b = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int pb = 0, pt = 0;
    for (int c = threadIdx.x; c < nchunks; c += TPB) {
        const int n = chunk_count[(size_t)b * nchunks + c];
        pt += n;
        if (c < chunk) pb += n;
    }
    before[threadIdx.x] = pb;
    total[threadIdx.x] = pt;
    __syncthreads();
    for (int off = TPB / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            before[threadIdx.x] += before[threadIdx.x + off];
            total[threadIdx.x] += total[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (chunk == 0 && threadIdx.x == 0) count[b] = total[0];

    const float* vb = v + (size_t)b * HW;
    const int base = chunk * NZ_CHUNK + wave * (NZ_ITERS * 64);
    unsigned long long m[NZ_ITERS];
    int n = 0;
#pragma unroll
    for (int it = 0; it < NZ_ITERS; ++it) {
        m[it] = nz_ballot(vb, HW, base + it * 64 + lane);
        n += __popcll(m[it]);
    }
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    int pos = before[0];
    for (int k = 0; k < wave; ++k) pos += wsum[k];
    int32_t* ib = index + (size_t)b * HW;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int it = 0; it < NZ_ITERS; ++it) {
        const int at = pos + __popcll(m[it] & below);
        if ((m[it] >> lane & 1ull) && at < HW) ib[at] = base + it * 64 + lane;
        pos += __popcll(m[it]);
    }
}

// ---- (d) the random sparse sample of the ground truth -----------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
sample_init_kernel(const float* __restrict__ depth, const int32_t* __restrict__ nsel, float* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= HW) return;
    out[(size_t)b * HW + i] = nsel[b] < 0 ? depth[(size_t)b * HW + i] : 0.f;      // depth_tensor.clone() / zeros_like
}

__global__ void __launch_bounds__(TPB)
sample_scatter_kernel(const float* __restrict__ depth, const int32_t* __restrict__ index, const int32_t* __restrict__ perm,
                      const int32_t* __restrict__ sel_off, const int32_t* __restrict__ nsel, float* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= nsel[b]) return;
    const int r = perm[sel_off[b] + j];                             // a rank among the image's non-zero pixels
    if (r < 0 || r >= HW) return;
    const int p = index[(size_t)b * HW + r];
    if (p < 0 || p >= HW) return;
    out[(size_t)b * HW + p] = depth[(size_t)b * HW + p];
}

// ---- (e) NYU ground truth: nearest resize, / divisor, then the depth range ---------------------------------------------------------
__global__ void __launch_bounds__(TPB)
nearest_u16_depth_range_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int H, int W, int Ho, int Wo,
                               const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab, float divisor, float min_depth,
                               float max_depth) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= Ho * Wo) return;
    const int yo = idx / Wo, xo = idx - yo * Wo;
    const int ys = ytab[yo], xs = xtab[xo];
    const float v = (ys >= 0 && ys < H && xs >= 0 && xs < W) ? (float)src[((size_t)b * H + ys) * W + xs] : 0.f;
    float d = __fdiv_rn(v, divisor);
    if (d < min_depth) d = 0.f;                                     // depth_tensor[depth_tensor < self.min_depth] = 0
    if (d > max_depth) d = 0.f;
    dst[(size_t)b * Ho * Wo + idx] = d;
}

inline bool fits_int(long long n) { return n > 0 && n <= 0x7fffffffLL; }

}  // namespace

extern "C" int vidc_u8_decode_chw(const uint8_t* src_hwc, float* dst_chw, int B, int H, int W, int C, int mode, vidc_stream_t stream) {
    VIDC_REQUIRE(src_hwc && dst_chw, VIDC_ERR_NULL, "vidc_u8_decode_chw: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (C == 1 || C == 3) && mode >= 0 && mode <= 3 && fits_int((long long)H * W * C),
                 VIDC_ERR_SHAPE, "vidc_u8_decode_chw: bad shape (B %d, H %d, W %d, C %d (1 or 3), mode %d (0..3))", B, H, W, C, mode);
    const int HW = H * W;
    hipStream_t st = vidc::as_stream(stream);
    if (HW % 16 == 0 && ((uintptr_t)src_hwc & 15) == 0 && ((uintptr_t)dst_chw & 15) == 0) {
        dim3 grid((HW / 16 + TPB - 1) / TPB, B, 1);
        if (C == 3) hipLaunchKernelGGL(u8_decode_vec_kernel<3>, grid, dim3(TPB), 0, st, src_hwc, dst_chw, HW, mode);
        else hipLaunchKernelGGL(u8_decode_vec_kernel<1>, grid, dim3(TPB), 0, st, src_hwc, dst_chw, HW, mode);
        VIDC_CHECK_LAUNCH("u8_decode_vec_kernel");
    } else {
        dim3 grid((unsigned)(((long long)HW * C + TPB - 1) / TPB), B, 1);
        hipLaunchKernelGGL(u8_decode_scalar_kernel, grid, dim3(TPB), 0, st, src_hwc, dst_chw, HW, C, mode);
        VIDC_CHECK_LAUNCH("u8_decode_scalar_kernel");
    }
    return VIDC_OK;
}

extern "C" size_t vidc_rasterize_pixel_tracks_scratch_bytes(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 ? (size_t)B * H * W * sizeof(int32_t) : 0;
}

extern "C" int vidc_rasterize_pixel_tracks(const double* tracks, const int32_t* offsets, int n_tracks, int B, double divisor,
                                           const float* gt_depth, float* depth, int H, int W, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(offsets && depth && scratch && (tracks || n_tracks == 0), VIDC_ERR_NULL, "vidc_rasterize_pixel_tracks: null pointer");
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && n_tracks >= 0 && n_tracks <= 0x7fffffff - TPB && fits_int((long long)B * H * W) &&
                     divisor == divisor && divisor != 0.0,
                 VIDC_ERR_SHAPE, "vidc_rasterize_pixel_tracks: bad shape (B %d, H %d, W %d, %d tracks, divisor %g)", B, H, W, n_tracks, divisor);
    hipStream_t st = vidc::as_stream(stream);
    const long long n = (long long)B * H * W;
    int32_t* winner = static_cast<int32_t*>(scratch);
    hipLaunchKernelGGL(tracks_clear_kernel, dim3(vidc::blocks(n)), dim3(TPB), 0, st, winner, n);
    VIDC_CHECK_LAUNCH("tracks_clear_kernel");
    if (n_tracks > 0) {
        hipLaunchKernelGGL(tracks_vote_kernel, dim3(vidc::blocks(n_tracks)), dim3(TPB), 0, st, tracks, offsets, n_tracks, B, divisor, winner, H, W);
        VIDC_CHECK_LAUNCH("tracks_vote_kernel");
    }
    hipLaunchKernelGGL(tracks_write_kernel, dim3(vidc::blocks(n)), dim3(TPB), 0, st, tracks, winner, gt_depth, depth, n, n_tracks);
    VIDC_CHECK_LAUNCH("tracks_write_kernel");
    return VIDC_OK;
}

extern "C" size_t vidc_nonzero_compact_scratch_bytes(int B, int HW) {
    return B > 0 && HW > 0 ? (size_t)B * vidc::cdiv(HW, NZ_CHUNK) * sizeof(int32_t) : 0;
}

extern "C" int vidc_nonzero_compact(const float* v, int B, int HW, int32_t* count, int32_t* index, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(v && count && index && scratch, VIDC_ERR_NULL, "vidc_nonzero_compact: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW <= 0x7fffffff - NZ_CHUNK, VIDC_ERR_SHAPE, "vidc_nonzero_compact: bad shape (B %d, HW %d)", B, HW);
    hipStream_t st = vidc::as_stream(stream);
    const int nchunks = vidc::cdiv(HW, NZ_CHUNK);
    int32_t* chunk_count = static_cast<int32_t*>(scratch);
    dim3 grid(nchunks, B, 1);
    hipLaunchKernelGGL(nonzero_count_kernel, grid, dim3(TPB), 0, st, v, HW, nchunks, chunk_count);
    VIDC_CHECK_LAUNCH("nonzero_count_kernel");
    hipLaunchKernelGGL(nonzero_scatter_kernel, grid, dim3(TPB), 0, st, v, HW, nchunks, chunk_count, count, index);
    VIDC_CHECK_LAUNCH("nonzero_scatter_kernel");
    return VIDC_OK;
}

extern "C" int vidc_sparse_sample_scatter(const float* depth, const int32_t* index, const int32_t* perm, const int32_t* sel_off,
                                          const int32_t* nsel, int max_sel, int B, int HW, float* out, vidc_stream_t stream) {
    VIDC_REQUIRE(depth && index && sel_off && nsel && out && (perm || max_sel == 0), VIDC_ERR_NULL, "vidc_sparse_sample_scatter: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW <= 0x7fffffff - TPB && max_sel >= 0 && max_sel <= HW, VIDC_ERR_SHAPE,
                 "vidc_sparse_sample_scatter: bad shape (B %d, HW %d, max_sel %d)", B, HW, max_sel);
    hipStream_t st = vidc::as_stream(stream);
    hipLaunchKernelGGL(sample_init_kernel, dim3(vidc::blocks(HW), B, 1), dim3(TPB), 0, st, depth, nsel, out, HW);
    VIDC_CHECK_LAUNCH("sample_init_kernel");
    if (max_sel > 0) {
        hipLaunchKernelGGL(sample_scatter_kernel, dim3(vidc::blocks(max_sel), B, 1), dim3(TPB), 0, st, depth, index, perm, sel_off, nsel, out, HW);
        VIDC_CHECK_LAUNCH("sample_scatter_kernel");
    }
    return VIDC_OK;
}

extern "C" int vidc_resize_nearest_u16_depth_range(const uint16_t* src, float* dst, int B, int H, int W, int Ho, int Wo, const int32_t* xtab,
                                                   const int32_t* ytab, float divisor, float min_depth, float max_depth, vidc_stream_t stream) {
    VIDC_REQUIRE(src && dst && xtab && ytab, VIDC_ERR_NULL, "vidc_resize_nearest_u16_depth_range: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && fits_int((long long)Ho * Wo) && divisor != 0.f && min_depth <= max_depth,
                 VIDC_ERR_SHAPE, "vidc_resize_nearest_u16_depth_range: bad shape or range");
    dim3 grid((Ho * Wo + TPB - 1) / TPB, B, 1);
    hipLaunchKernelGGL(nearest_u16_depth_range_kernel, grid, dim3(TPB), 0, vidc::as_stream(stream), src, dst, H, W, Ho, Wo, xtab, ytab, divisor,
                       min_depth, max_depth);
    VIDC_CHECK_LAUNCH("nearest_u16_depth_range_kernel");
    return VIDC_OK;
}
