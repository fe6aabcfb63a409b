// What the two PNG writers share (png.hip: stored deflate blocks; png_deflate.hip: filters and one Huffman block): the geometry of a file, the
// sample conversions, CRC-32 as polynomial arithmetic, the wave sums and the 43 bytes in front of the deflate data.
#pragma once
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

// The 43 bytes in front of the deflate data: signature, IHDR with its CRC, the IDAT length (zlen: the zlib stream's bytes) and type, 78 01
__device__ inline void png_head(uint8_t* out, const PngGeom& g, uint32_t zlen) {
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
}

}  // namespace
