// The evaluation outputs as PNG files, written on the device (SaveNormalsToImage / SaveDepthsToImage / SaveMasksToImage / SaveRgbToImage,
// network_run.py:32-69; the --save side of _network_save_cnn_evaluation_output / _network_save_cnn_output_pred_only, :261-292).
//
// A PNG whose deflate stream holds only STORED blocks needs no entropy coder: the file is a byte layout plus an Adler-32 over the raw
// scanlines and a CRC-32 over the IDAT chunk, and both checksums are sums over segments (include/vidc.h states the layout byte for byte).
//
//   launch 1 (file segments x images): a workgroup owns 4096 consecutive FILE bytes (16 per lane, 16-byte aligned) of the region that the
//       block headers and the scanlines occupy, [43, E).  It converts the samples lane-per-byte into LDS (consecutive lanes read
//       consecutive addresses of one plane), stores its lane's 16 bytes (one dwordx4; dwords and bytes at the two ends of the region) and
//       leaves three numbers per segment: a = sum of its raw bytes, b = sum of (raw bytes after this one in the segment + 1) * byte, and
//       p = the CRC register after its file bytes started from 0.
//   launch 2 (one workgroup per image): folds the partials -- with rest_i the raw bytes and after_i the file bytes of the region behind
//       segment i: A = 1 + sum a_i, B = raw + sum (b_i + a_i rest_i) (mod 65521), body = xor p_i x^(8 after_i) (mod P) -- and writes
//       everything outside the region: signature, IHDR, the IDAT length / type / zlib header, the Adler bytes, the IDAT CRC, IEND.
//
// The seam between the two is the kernel boundary: nothing is handed between workgroups inside a launch.  Every sum is an exact integer
// or GF(2) sum, so the bytes of an image depend on nothing but the image: not on B, on the grid or on the stride between the files.
#include "common.h"
#include <cstdint>

namespace {

constexpr int PT = 256;                    // threads per workgroup
constexpr uint32_t SEG = 16 * PT;          // file bytes per workgroup
constexpr uint32_t SEG0 = 32;              // file offset of segment 0 (16-byte aligned; the region starts inside it)
constexpr uint32_t BODY0 = 43;             // signature 8 + IHDR 25 + IDAT length and type 8 + zlib header 2: the first block header
constexpr uint32_t BLK = 65535;            // raw bytes of every stored block but the last
constexpr uint32_t BLKH = BLK + 5;         // ... with its header
constexpr uint32_t POLY = 0xEDB88320u;     // CRC-32, reflected
constexpr uint32_t ADLER = 65521u;

struct PngGeom {
    uint32_t H, W, rowbytes, raw, nblocks, body_end, nseg, bitdepth, colourtype;      // body_end = E: the file offset of the Adler bytes
};

// H, W > 0, a known format and an IDAT chunk within PNG's 2^31 - 1 bytes (so every file offset fits 32 bits)
bool png_geom(int H, int W, int format, PngGeom& g) {
    if (H <= 0 || W <= 0 || format < VIDC_PNG_DEPTH16_F32 || format > VIDC_PNG_GRAY8_U8) return false;
    const uint64_t bpp = format == VIDC_PNG_DEPTH16_F32 ? 2 : format == VIDC_PNG_GRAY8_U8 ? 1 : 3;
    const uint64_t rowbytes = 1 + (uint64_t)W * bpp, raw = (uint64_t)H * rowbytes, nblocks = (raw + BLK - 1) / BLK;
    if (2 + 5 * nblocks + raw + 4 > 0x7FFFFFFFull) return false;
    g.H = (uint32_t)H, g.W = (uint32_t)W, g.rowbytes = (uint32_t)rowbytes, g.raw = (uint32_t)raw, g.nblocks = (uint32_t)nblocks;
    g.body_end = (uint32_t)(BODY0 + 5 * nblocks + raw);
    g.nseg = (g.body_end - SEG0 + SEG - 1) / SEG;
    g.bitdepth = format == VIDC_PNG_DEPTH16_F32 ? 16 : 8;
    g.colourtype = format == VIDC_PNG_NORMAL8_F32 || format == VIDC_PNG_RGB8_F32 ? 2 : 0;
    return true;
}

// a * b mod P on reflected polynomials (bit 31 = x^0): zlib's multmodp in 32 fixed steps
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

struct PowTables {
    uint32_t x8n[32];       // x^(8 * 2^j): what 2^j further bytes do to a CRC register
    uint32_t slice[PT];     // x^(8 * 16 * k): k further 16-byte lane slices
    constexpr PowTables() : x8n{}, slice{} {
        uint32_t p = 0x40000000u;                      // x^1
        for (int i = 0; i < 3; ++i) p = mulmod(p, p);
        for (int j = 0; j < 32; ++j) x8n[j] = p, p = mulmod(p, p);
        slice[0] = 0x80000000u;                        // x^0
        for (int k = 1; k < PT; ++k) slice[k] = mulmod(slice[k - 1], x8n[4]);
    }
};
__constant__ PowTables kPow{};

__device__ inline uint32_t xpow8(uint32_t nbytes) {       // x^(8 * nbytes) mod P
    uint32_t p = 0x80000000u;
    for (int j = 0; nbytes; nbytes >>= 1, ++j)
        if (nbytes & 1u) p = mulmod(kPow.x8n[j], p);
    return p;
}

__device__ inline uint32_t crc_bits(uint32_t s, uint32_t byte) {      // one byte through the register without a table (launch 2's few bytes)
    s ^= byte;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = (s >> 1) ^ (POLY & (0u - (s & 1u)));
    return s;
}

// raw bytes at file offsets below f, BODY0 <= f <= E
__device__ inline uint32_t raw_below(uint32_t f) {
    const uint32_t u = f - BODY0, k = u / BLKH, m = u - k * BLKH;
    return k * BLK + (m > 5 ? m - 5 : 0);
}

__device__ inline uint32_t clamp_u8(float t) { return !(t > 0.f) ? 0u : t >= 255.f ? 255u : (uint32_t)t; }      // truncation; NaN -> 0

// raw byte i of one image: the filter byte 0 in front of every row, then the row's samples
template <int FMT>
__device__ inline uint32_t raw_byte(const void* __restrict__ img, uint32_t i, const PngGeom& g, size_t HW) {
    const uint32_t r = i / g.rowbytes, c = i - r * g.rowbytes;
    if (c == 0) return 0;
    const size_t row = (size_t)r * g.W;
    if (FMT == VIDC_PNG_GRAY8_U8) return static_cast<const uint8_t*>(img)[row + (c - 1)];
    const float* f = static_cast<const float*>(img);
    if (FMT == VIDC_PNG_DEPTH16_F32) {           // depth_to_mm_kernel (metrics.hip), then Pillow's saturating I -> I;16, big-endian
        const float v = __fmul_rn(f[row + ((c - 1) >> 1)], 1000.0f);
        const uint32_t mm = v >= 65535.0f ? 65535u : (v > 0.f ? (uint32_t)v : 0u);
        return ((c - 1) & 1u) ? (mm & 255u) : (mm >> 8);
    }
    const uint32_t px = (c - 1) / 3, ch = (c - 1) - 3 * px;
    const float x = f[ch * HW + row + px];
    // (1 + n) * 127.5 in two rounded operations like numpy: the fused form gives another byte at n = k / 127.5 - 1 for some k
    return clamp_u8(FMT == VIDC_PNG_NORMAL8_F32 ? __fmul_rn(__fadd_rn(1.0f, x), 127.5f) : __fmul_rn(x, 255.0f));
}

__device__ inline uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v ^= (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}
__device__ inline uint32_t wave_add(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}
__device__ inline unsigned long long wave_add(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// partial[b * nseg + s] = (a, b, p, 0) of segment s of image b; the segment's bytes of files + b * file_stride
template <int FMT>
__global__ void __launch_bounds__(PT)
png_payload_kernel(const void* __restrict__ src, uint8_t* __restrict__ files, size_t file_stride, uint4* __restrict__ partial, PngGeom g) {
    __shared__ uint4 seg[PT];                  // the segment's 4096 file bytes
    __shared__ uint32_t tab[256];              // byte-wise CRC table
    __shared__ uint32_t red[3][PT / 64];
    __shared__ uint32_t last_p;
    const uint32_t t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const size_t HW = (size_t)g.H * g.W;
    const void* img = FMT == VIDC_PNG_GRAY8_U8 ? static_cast<const void*>(static_cast<const uint8_t*>(src) + b * HW)
                                               : static_cast<const void*>(static_cast<const float*>(src) + b * HW * (FMT == VIDC_PNG_DEPTH16_F32 ? 1 : 3));
    uint8_t* file = files + b * file_stride;
    {
        uint32_t c = t;
#pragma unroll
        for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (POLY & (0u - (c & 1u)));
        tab[t] = c;
    }
    // ---- bytes: lane-per-byte, so that consecutive lanes read consecutive samples of a plane
    const uint32_t f_seg = SEG0 + s * SEG;
    uint8_t* segb = reinterpret_cast<uint8_t*>(seg);
#pragma unroll 4
    for (uint32_t j = t; j < SEG; j += PT) {
        const uint32_t f = f_seg + j;
        uint32_t v = 0;
        if (f >= BODY0 && f < g.body_end) {
            const uint32_t u = f - BODY0, k = u / BLKH, m = u - k * BLKH;
            if (m < 5) {                       // BFINAL, LEN, ~LEN (little-endian)
                const uint32_t fin = k + 1 == g.nblocks, len = fin ? g.raw - k * BLK : BLK;
                v = m == 0 ? fin : ((m < 3 ? len : ~len) >> (8 * ((m - 1) & 1u))) & 255u;
            } else {
                v = raw_byte<FMT>(img, k * BLK + (m - 5), g, HW);
            }
        }
        segb[j] = (uint8_t)v;
    }
    __syncthreads();
    // ---- this lane's 16 bytes [f0, f0 + 16) cut to the region: [lo, hi)
    const uint32_t f0 = f_seg + 16 * t, seg_end = min(f_seg + SEG, g.body_end);
    const uint32_t lo = max(f0, BODY0), hi = min(f0 + 16, g.body_end);
    const uint4 q = seg[t];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if (lo == f0 && hi == f0 + 16) {
        *reinterpret_cast<uint4*>(file + f0) = q;
    } else if (lo < hi) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t fd = f0 + 4 * d;
            if (fd >= lo && fd + 4 <= hi) {
                *reinterpret_cast<uint32_t*>(file + fd) = w[d];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (fd + e >= lo && fd + e < hi) file[fd + e] = (uint8_t)(w[d] >> (8 * e));
            }
        }
    }
    // ---- this lane's sums: CRC register from 0 over its file bytes, Adler pair from (0, 0) over its raw bytes
    uint32_t crc = 0, al = 0, bl = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t f = f0 + e;
        if (f >= lo && f < hi) {
            const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 255u;
            crc = tab[(crc ^ byte) & 255u] ^ (crc >> 8);
            if ((f - BODY0) % BLKH >= 5) al += byte, bl += al;
        }
    }
    // ---- the segment's: lane t's bytes are followed by those of the lanes up to tl, whose slice holds the last `tail` bytes
    const uint32_t tl = (seg_end - 1 - f_seg) >> 4, tail = seg_end - f_seg - 16 * tl;
    const uint32_t fe = min(max(f0 + 16, BODY0), seg_end);
    const uint32_t bs = bl + al * (raw_below(seg_end) - raw_below(fe));           // < 2^32: at most 4096 raw bytes per segment
    uint32_t p = t < tl ? mulmod(crc, kPow.slice[tl - t - 1]) : 0u;               // ... x^(8 * tail) below
    if (t == tl) last_p = crc;
    p = wave_xor(p);
    const uint32_t a_w = wave_add(al), b_w = wave_add(bs);
    if ((t & 63) == 0) red[0][t >> 6] = a_w, red[1][t >> 6] = b_w, red[2][t >> 6] = p;
    __syncthreads();
    if (t == 0) {
        const uint32_t px = red[2][0] ^ red[2][1] ^ red[2][2] ^ red[2][3];
        partial[(size_t)b * g.nseg + s] = make_uint4(red[0][0] + red[0][1] + red[0][2] + red[0][3], red[1][0] + red[1][1] + red[1][2] + red[1][3],
                                                     mulmod(px, xpow8(tail)) ^ last_p, 0u);
    }
}

__global__ void __launch_bounds__(PT)
png_close_kernel(const uint4* __restrict__ partial, uint8_t* __restrict__ files, size_t file_stride, PngGeom g) {
    __shared__ unsigned long long red64[2][PT / 64];
    __shared__ uint32_t red32[PT / 64];
    __shared__ uint8_t out[BODY0 + 20];        // the 43 bytes in front of the region, the 20 behind it
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    unsigned long long A = 0, B = 0;
    uint32_t body = 0;
    for (uint32_t i = t; i < g.nseg; i += PT) {
        const uint4 v = partial[(size_t)b * g.nseg + i];
        const uint32_t seg_end = min(SEG0 + (i + 1) * SEG, g.body_end);
        A += v.x;
        B += (v.y + (unsigned long long)v.x * (g.raw - raw_below(seg_end))) % ADLER;
        body ^= mulmod(v.z, xpow8(g.body_end - seg_end));
    }
    A = wave_add(A), B = wave_add(B), body = wave_xor(body);
    if ((t & 63) == 0) red64[0][t >> 6] = A, red64[1][t >> 6] = B, red32[t >> 6] = body;
    __syncthreads();
    if (t == 0) {
        A = (1 + red64[0][0] + red64[0][1] + red64[0][2] + red64[0][3]) % ADLER;
        B = (g.raw + red64[1][0] + red64[1][1] + red64[1][2] + red64[1][3]) % ADLER;
        const uint32_t adler = (uint32_t)B << 16 | (uint32_t)A, zlen = g.body_end - BODY0 + 2 + 4;
        const uint8_t head[BODY0] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                     (uint8_t)(g.W >> 24), (uint8_t)(g.W >> 16), (uint8_t)(g.W >> 8), (uint8_t)g.W,
                                     (uint8_t)(g.H >> 24), (uint8_t)(g.H >> 16), (uint8_t)(g.H >> 8), (uint8_t)g.H,
                                     (uint8_t)g.bitdepth, (uint8_t)g.colourtype, 0, 0, 0, 0, 0, 0, 0,
                                     (uint8_t)(zlen >> 24), (uint8_t)(zlen >> 16), (uint8_t)(zlen >> 8), (uint8_t)zlen, 'I', 'D', 'A', 'T', 0x78, 0x01};
        for (uint32_t i = 0; i < BODY0; ++i) out[i] = head[i];
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 12; i < 29; ++i) c = crc_bits(c, out[i]);
        c = ~c;
        out[29] = (uint8_t)(c >> 24), out[30] = (uint8_t)(c >> 16), out[31] = (uint8_t)(c >> 8), out[32] = (uint8_t)c;
        // IDAT: the type and the zlib header, then the region through its folded partials, then the Adler bytes
        c = 0xFFFFFFFFu;
        for (uint32_t i = 37; i < BODY0; ++i) c = crc_bits(c, out[i]);
        c = mulmod(c, xpow8(g.body_end - BODY0)) ^ red32[0] ^ red32[1] ^ red32[2] ^ red32[3];
        uint8_t* tailb = out + BODY0;
        tailb[0] = (uint8_t)(adler >> 24), tailb[1] = (uint8_t)(adler >> 16), tailb[2] = (uint8_t)(adler >> 8), tailb[3] = (uint8_t)adler;
        for (int i = 0; i < 4; ++i) c = crc_bits(c, tailb[i]);
        c = ~c;
        tailb[4] = (uint8_t)(c >> 24), tailb[5] = (uint8_t)(c >> 16), tailb[6] = (uint8_t)(c >> 8), tailb[7] = (uint8_t)c;
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) tailb[8 + i] = iend[i];
    }
    __syncthreads();
    uint8_t* file = files + b * file_stride;
    if (t < BODY0) file[t] = out[t];
    else if (t < BODY0 + 20) file[g.body_end + (t - BODY0)] = out[t];
}

}  // namespace

extern "C" size_t vidc_png_file_bytes(int H, int W, int format) {
    PngGeom g;
    return png_geom(H, W, format, g) ? (size_t)g.body_end + 20 : 0;
}

extern "C" size_t vidc_png_scratch_bytes(int B, int H, int W, int format) {
    PngGeom g;
    return B > 0 && png_geom(H, W, format, g) ? (size_t)B * g.nseg * sizeof(uint4) : 0;
}

extern "C" int vidc_png_encode(const void* src, int B, int H, int W, int format, uint8_t* files, size_t file_stride, void* scratch,
                               vidc_stream_t stream) {
    VIDC_REQUIRE(src && files && scratch, VIDC_ERR_NULL, "vidc_png_encode: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, VIDC_ERR_SHAPE, "vidc_png_encode: bad shape B=%d H=%d W=%d", B, H, W);
    VIDC_REQUIRE(format >= VIDC_PNG_DEPTH16_F32 && format <= VIDC_PNG_GRAY8_U8, VIDC_ERR_SHAPE, "vidc_png_encode: unknown format %d", format);
    PngGeom g;
    VIDC_REQUIRE(png_geom(H, W, format, g), VIDC_ERR_SHAPE, "vidc_png_encode: a %dx%d image does not fit one IDAT chunk (2^31 - 1 bytes)", H, W);
    VIDC_REQUIRE(file_stride >= (size_t)g.body_end + 20 && file_stride % 16 == 0 && reinterpret_cast<uintptr_t>(files) % 16 == 0, VIDC_ERR_SHAPE,
                 "vidc_png_encode: file_stride %zu must be a multiple of 16 and at least the %zu bytes of a file, files 16-byte aligned",
                 file_stride, (size_t)g.body_end + 20);
    VIDC_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, VIDC_ERR_SHAPE, "vidc_png_encode: scratch must be 16-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    uint4* partial = static_cast<uint4*>(scratch);
    const dim3 grid(g.nseg, B);
    switch (format) {
        case VIDC_PNG_DEPTH16_F32: hipLaunchKernelGGL(png_payload_kernel<VIDC_PNG_DEPTH16_F32>, grid, dim3(PT), 0, st, src, files, file_stride, partial, g); break;
        case VIDC_PNG_NORMAL8_F32: hipLaunchKernelGGL(png_payload_kernel<VIDC_PNG_NORMAL8_F32>, grid, dim3(PT), 0, st, src, files, file_stride, partial, g); break;
        case VIDC_PNG_RGB8_F32: hipLaunchKernelGGL(png_payload_kernel<VIDC_PNG_RGB8_F32>, grid, dim3(PT), 0, st, src, files, file_stride, partial, g); break;
        default: hipLaunchKernelGGL(png_payload_kernel<VIDC_PNG_GRAY8_U8>, grid, dim3(PT), 0, st, src, files, file_stride, partial, g); break;
    }
    VIDC_CHECK_LAUNCH("png_payload_kernel");
    hipLaunchKernelGGL(png_close_kernel, dim3(B), dim3(PT), 0, st, partial, files, file_stride, g);
    VIDC_CHECK_LAUNCH("png_close_kernel");
    return VIDC_OK;
}
