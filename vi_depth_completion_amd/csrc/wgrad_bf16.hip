// Weight gradient of a conv in bf16 on the matrix cores, in one launch plus the shared final reduction (wgrad_final.h):
//   dW[co][ci][kh][kw] = sum_m q(dY[m][co]) * q(X[pixel(m) shifted by the tap][ci]),   q = bf16_rne
// It reads the fp32 NHWC tensors autograd already holds, rounds them on the way into LDS and runs v_mfma_f32_32x32x16_bf16 with the pixel as
// the reduction index: no cast, transposed or im2col tensor ever reaches HBM (the captured trainers' bf16 chain writes all three).
//
// Grid = (co tile of 128, ci tile of 128 x tap, pixel chunk), the grid of train.hip's fp32 wgrad_kernel, so the scratch layout
// [chunk][tap][Cout][Cin] and wgrad_final_kernel are shared.  Per step of 32 pixels the 256 threads stage two tiles, dY[32 px][128 co] and
// the tap-shifted X[32 px][128 ci], with 16-byte global loads into two LDS images of 256-byte rows (pixels past the chunk, taps outside the
// image and channels past Cout / Cin are stored as zeros: pad, don't mask).  Both operands are pixel-major there and the MFMA wants them
// pixel-minor (A = dY^T: co x pixels, B = X: pixels x ci), which is what gfx950's transposed LDS read delivers: one ds_read_b64_tr_b16 hands a
// lane the four pixels 4n .. 4n+3 of ITS channel.  The sum over pixels does not care which of a k-step's 16 pixels sits in which fragment
// element as long as A and B agree, so lane half h takes pixels 8h .. 8h+7 of the k-step in the order the two reads deliver them.
// Each wave owns a 64 x 64 (co, ci) register tile = 2 x 2 MFMA tiles; the images are double-buffered, the next step's global loads are in
// flight under the MFMAs of the current one, and there is one barrier per step.
#include "common.h"
#include "train_rows.h"
#include "wgrad_final.h"
#include <cstdint>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) i16x4 lds_i16x4;

constexpr int kStep = 32;                       // pixels per staged tile = two k-steps of the MFMA
constexpr int kImage = kStep * 256;             // bytes of one [32 px][128 x bf16] image
constexpr int kMaxRows = 1024;                  // pixels per chunk at most (fp32 accumulation chain, see rows_per_chunk)

// Byte offset of 16-byte unit `ch` (8 channels) of pixel row `row` in an image: 256-byte rows, the unit index XORed with the row so that both
// the 16-byte staging stores and the transposed reads below are free of bank conflicts -- by the bank rule, not yet by a counter run.  A
// 32-lane half of a transposed read takes 4 rows x 4 units (64 bytes per row): the row's low two bits move the four units to a different
// 64-byte quarter of the 64 banks.
__device__ inline unsigned image_off(int row, int ch) { return 256u * (unsigned)row + 16u * (unsigned)(ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

__device__ inline bf16x8 read_tr_pair(const unsigned char* lds, unsigned a0, unsigned a1) {
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(lds + a0));
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(lds + a1));
    const i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ void __launch_bounds__(256)
wgrad_bf16_kernel(const float* __restrict__ dy, const float* __restrict__ x, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int lddy,
                  int KH, int KW, int stride, int pad, int dil, int rows_per_chunk, float* __restrict__ partial /* [chunk][tap][Cout][Cin] */) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kImage];      // [buffer][dY image | X image]
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                  // scalar: what depends on it branches without touching EXEC
    const int taps = KH * KW;
    const int ci_tiles = (Cin + 127) / 128;
    const int tap = blockIdx.y / ci_tiles, cit = blockIdx.y - tap * ci_tiles;
    const int kh = tap / KW, kw = tap - kh * KW;
    const int coT = blockIdx.x * 128, ciT = cit * 128;
    const long long M = (long long)B * Ho * Wo;
    const long long m_begin = (long long)blockIdx.z * rows_per_chunk, m_end = min(M, m_begin + rows_per_chunk);
    const int m_lo = (int)m_begin, m_hi = (int)m_end;                           // (32-bit offsets: the host checks both tensors stay below 2^31 elements)

    // ---- staging: thread -> 8 channels (one 16-byte unit of bf16) of pixel rows srow and srow + 16 of the step ----
    const int srow = tid >> 4, sch = tid & 15;
    const int co_s = coT + sch * 8, ci_s = ciT + sch * 8;
    const bool a_ok0 = co_s < Cout, a_ok1 = co_s + 4 < Cout, b_ok0 = ci_s < Cin, b_ok1 = ci_s + 4 < Cin;      // Cout, Cin are multiples of 4
    // (b, oy, ox) of the chunk's first pixel is decoded once (uniform) and every thread walks from there with compares, like wgrad_kernel
    int ox0 = m_lo % Wo + srow, oy0 = (m_lo / Wo) % Ho, b0 = m_lo / (Wo * Ho);
    while (ox0 >= Wo) { ox0 -= Wo; ++oy0; }
    while (oy0 >= Ho) { oy0 -= Ho; ++b0; }
    float ra[2][8], rx[2][8];
    auto gload = [&](int m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + srow + 16 * i;
            int ox = ox0 + 16 * i, oy = oy0, b = b0;
            while (ox >= Wo) { ox -= Wo; ++oy; }
            while (oy >= Ho) { oy -= Ho; ++b; }
#pragma unroll
            for (int k = 0; k < 8; ++k) ra[i][k] = rx[i][k] = 0.f;
            if (m < m_hi) {
                const float* pa = dy + m * lddy + co_s;
                if (a_ok0) vidc::load4(pa, ra[i]);
                if (a_ok1) vidc::load4(pa + 4, ra[i] + 4);
                const int iy = oy * stride - pad + kh * dil, ix = ox * stride - pad + kw * dil;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                    const float* px = x + ((b * H + iy) * W + ix) * ldx + ci_s;
                    if (b_ok0) vidc::load4(px, rx[i]);
                    if (b_ok1) vidc::load4(px + 4, rx[i] + 4);
                }
            }
        }
        ox0 += kStep;
        while (ox0 >= Wo) { ox0 -= Wo; ++oy0; }
        while (oy0 >= Ho) { oy0 -= Ho; ++b0; }
    };
    const unsigned st_off[2] = {image_off(srow, sch), image_off(srow + 16, sch)};
    auto stage = [&](int buf) {
        unsigned char* img = lds + buf * 2 * kImage;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            vidc::store8_bf16(reinterpret_cast<unsigned short*>(img + st_off[i]), ra[i]);
            vidc::store8_bf16(reinterpret_cast<unsigned short*>(img + kImage + st_off[i]), rx[i]);
        }
    };

    // ---- fragments: wave -> 64 co x 64 ci; a wave whose tile lies past Cout or Cin only stages ----
    const int wco = (wave >> 1) * 64, wci = (wave & 1) * 64;
    const bool live = coT + wco < Cout && ciT + wci < Cin;                      // scalar
    // Transposed read of k-step kk, read n: the lane's 16-lane group g = lane >> 4 takes the block of pixel rows 16 kk + 8 lh + 4 n .. + 3 and
    // the 16 channels 32 sub + 16 (g & 1) .. + 15 of the wave's 64; lane 4 q + p of the group supplies the address of row q, channels 4 p .. 4 p + 3.
    const int gq = (lane & 15) >> 2, gp = lane & 3, gcol = 2 * ((lane >> 4) & 1) + (gp >> 1);
    unsigned fa[2][2], fb[2][2];                                                // [n][sub], k-step 0 (k-step 1: + 16 rows)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = 8 * lh + 4 * n + gq;
            fa[n][s] = image_off(row, wco / 8 + 4 * s + gcol) + 8u * (gp & 1);
            fb[n][s] = kImage + image_off(row, wci / 8 + 4 * s + gcol) + 8u * (gp & 1);
        }
    f32x16 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][q][r] = 0.f;

    const int steps = (m_hi - m_lo + kStep - 1) / kStep;                        // uniform: every thread reaches every barrier
    gload(m_lo);
    stage(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) gload(m_lo + (s + 1) * kStep);
        if (live) {                                                             // EXEC is all ones here: the branch is on a scalar
            const unsigned char* img = lds + (s & 1) * 2 * kImage;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = read_tr_pair(img + kk * 16 * 256, fa[0][t], fa[1][t]);
                    b[t] = read_tr_pair(img + kk * 16 * 256, fb[0][t], fb[1][t]);
                }
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[p], b[q], acc[p][q], 0, 0, 0);
            }
        }
        if (more) stage((s + 1) & 1);       // the buffer read in step s - 1: every wave has passed the barrier that ended it
        __syncthreads();
    }
    if (!live) return;
    // C/D layout: col j = lane & 31, row i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float* out = partial + ((size_t)blockIdx.z * taps + tap) * (size_t)Cout * Cin;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int cj = ciT + wci + q * 32 + li;
            if (cj >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = coT + wco + p * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ro < Cout) out[(size_t)ro * Cin + cj] = acc[p][q][r];
            }
        }
}

// Pixels per chunk: enough workgroups for 256 CUs like the fp32 entry, at least 256 pixels, at most 1024 -- short fp32 accumulation chains inside
// the MFMA, the chunk partials are then summed in fp64 (train.hip: wgrad_rows_per_chunk states the reason) -- and a multiple of the 32-pixel step.
inline int rows_per_chunk(long long M, int Cout, int Cin, int taps) {
    const long long tiles = (long long)((Cout + 127) / 128) * ((Cin + 127) / 128) * taps;
    const long long chunks = (1024 + tiles - 1) / tiles;
    long long rows = (M + chunks - 1) / chunks;
    if (rows < 256) rows = 256;
    if (rows > kMaxRows) rows = kMaxRows;
    rows = (rows + kStep - 1) / kStep * kStep;
    return (int)rows;
}

}  // namespace

extern "C" size_t vidc_conv_wgrad_bf16_scratch_bytes(int B, int Ho, int Wo, int Cout, int Cin, int KH, int KW) {
    const long long M = (long long)B * Ho * Wo;
    const int rows = rows_per_chunk(M, Cout, Cin, KH * KW);
    const long long chunks = (M + rows - 1) / rows;
    return (size_t)chunks * KH * KW * (size_t)Cout * Cin * sizeof(float);
}

extern "C" int vidc_conv_wgrad_bf16(const float* dy, const float* x, float* dw_oihw, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int lddy,
                                    int KH, int KW, int stride, int pad, int dilation, void* scratch, vidc_stream_t stream) {
    const char* what = "vidc_conv_wgrad_bf16";
    VIDC_REQUIRE(dy && x && dw_oihw && scratch, VIDC_ERR_NULL, "%s: null pointer", what);
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && dilation >= 1 && ldx >= Cin && lddy >= Cout,
                 VIDC_ERR_SHAPE, "%s: bad shape", what);
    VIDC_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0, VIDC_ERR_SHAPE,
                 "%s: Cin, Cout, ldx and lddy must be multiples of 4 (16-byte loads)", what);
    VIDC_REQUIRE(((uintptr_t)dy | (uintptr_t)x) % 16 == 0, VIDC_ERR_SHAPE, "%s: dy and x must be 16-byte aligned", what);
    VIDC_REQUIRE((long long)dilation * (KH - 1) <= H + 2 * pad - 1 && (long long)dilation * (KW - 1) <= W + 2 * pad - 1 &&
                     Ho == (H + 2 * pad - dilation * (KH - 1) - 1) / stride + 1 && Wo == (W + 2 * pad - dilation * (KW - 1) - 1) / stride + 1,
                 VIDC_ERR_SHAPE, "%s: Ho/Wo inconsistent", what);
    VIDC_REQUIRE((long long)B * H * W * ldx < (1ll << 31) && (long long)B * Ho * Wo * lddy < (1ll << 31), VIDC_ERR_SHAPE,
                 "%s: tensors must stay below 2^31 elements (32-bit offsets)", what);
    hipStream_t st = vidc::as_stream(stream);
    const long long M = (long long)B * Ho * Wo;
    const int taps = KH * KW;
    const int rows = rows_per_chunk(M, Cout, Cin, taps);
    const long long n_chunks = (M + rows - 1) / rows;
    VIDC_REQUIRE(n_chunks <= 65535, VIDC_ERR_SHAPE, "%s: %lld pixel chunks of %d pixels exceed the grid's 65535", what, n_chunks, rows);
    const int chunks = (int)n_chunks;
    float* partial = reinterpret_cast<float*>(scratch);
    hipLaunchKernelGGL(wgrad_bf16_kernel, dim3((Cout + 127) / 128, ((Cin + 127) / 128) * taps, chunks), dim3(256), 0, st, dy, x, B, H, W, Cin, ldx, Ho, Wo, Cout,
                       lddy, KH, KW, stride, pad, dilation, rows, partial);
    vidc::launch_wgrad_final(partial, chunks, taps, Cout, Cin, dw_oihw, st);
    VIDC_CHECK_LAUNCH("conv_wgrad_bf16");
    return VIDC_OK;
}
