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
#include "png_common.h"

namespace {

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
        png_head(out, g, zlen);
        // IDAT: the type and the zlib header, then the region through its folded partials, then the Adler bytes
        uint32_t c = 0xFFFFFFFFu;
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
