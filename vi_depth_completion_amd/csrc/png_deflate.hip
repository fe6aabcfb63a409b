// The evaluation outputs as COMPRESSED PNG files, written on the device: one of the five PNG filters per row, then ONE Huffman-only dynamic
// deflate block per image (include/vidc.h states the file bit for bit under `vidc_png_filter`).  No LZ77 and no run-length symbols: every
// filtered byte is one literal, so every step is a histogram, a scan or a table look-up.
//
//   launch 1 (row segments x images): a workgroup owns whole rows, about 4096 raw bytes (a longer row is one segment, walked in chunks of
//       4096).  It converts the samples of its rows and of the row above into LDS (raw_byte<FMT> of png_common.h), forms the five
//       candidates 16 bytes per lane, sums the five costs per row with LDS adds, chooses, and leaves in the scratch: the filtered bytes
//       (one dwordx4 per lane), a 256-bin histogram and the Adler pair (a, b) of the segment.
//   launch 2 (one workgroup per image): sums the histograms (end-of-block = 1), ranks the used symbols by (count, symbol), builds the code
//       lengths (Moffat-Katajainen in place on the sorted counts; beyond 15 bits zlib's repair of the length counts; a balanced code if
//       that ever costs more than the flat one), derives the canonical codes bit-reversed, scans the segments' bit counts (histogram .
//       lengths) into their bit offsets in the file, folds the Adler pairs, and writes the 43 + 138 bytes in front of the first symbol,
//       file_bytes[b] and the per-image numbers the next two launches read.
//   launch 3 (row segments x images): a segment looks its bytes up 16 per lane, scans the lanes' bit counts, ORs the codes into an LDS
//       image of its file dwords and stores whole dwords.  The byte two segments share belongs to the later one, which re-encodes the
//       at most seven symbols in front of its first; the last segment adds end-of-block, the pad bits and the Adler bytes.
//   launch 4 (one workgroup per image): CRC-32 over the IDAT type and data, whose length only the device knows, 16 bytes per lane per
//       pass, folded with mulmod / xpow8; the CRC and IEND.
//
// The seam between launches is the kernel boundary; inside a launch no workgroup reads what another one writes, and nothing is an atomic
// on global memory.  All arithmetic is integer or GF(2), so a file depends on its image and the filter mode alone.
#include "png_common.h"

namespace {

constexpr uint32_t CH = SEG;               // raw bytes per chunk: 16 per lane
constexpr uint32_t RMAX = PT;              // rows per segment at most: one lane chooses a row's filter
constexpr uint32_t NSYM = 257;             // 256 literals and end-of-block
constexpr uint32_t CODES = 260;            // stride of an image's code table in the scratch
constexpr uint32_t MAXBITS = 15;
constexpr uint32_t HDRBITS = 1106;         // 3 + 14 + 19 * 3 + 258 * 4: the first symbol's bit offset in the deflate data
constexpr uint32_t HDRLENS = 74;           // ... of which in front of the 258 lengths
constexpr uint32_t BUFW = CH * MAXBITS / 32 + 8;      // a chunk's bits as file dwords: + the offset in the first, end-of-block, pad, Adler

struct DeflGeom {
    PngGeom g;
    uint32_t rps, nseg, seg_cap;           // rows per segment, segments per image, bytes of a segment's slot in the scratch (16-byte multiple)
    uint64_t max_zlib;                     // the zlib stream under a flat 9-bit code: the bound of every image
};

bool defl_geom(int H, int W, int format, DeflGeom& d) {
    if (!png_geom(H, W, format, d.g)) return false;
    d.max_zlib = 2 + (HDRBITS + 9 * ((uint64_t)d.g.raw + 1) + 7) / 8 + 4;
    if (d.max_zlib > 0x7FFFFFFFull) return false;
    d.rps = d.g.rowbytes >= CH ? 1 : CH / d.g.rowbytes < RMAX ? CH / d.g.rowbytes : RMAX;
    d.nseg = (d.g.H + d.rps - 1) / d.rps;
    d.seg_cap = (uint32_t)(((uint64_t)d.rps * d.g.rowbytes + 15) / 16 * 16);
    return true;
}

// The scratch of B images, every part 16-byte aligned
struct DeflScratch {
    size_t filt, hist, adl, segbits, codes, meta, bytes;
};
DeflScratch defl_scratch(int B, const DeflGeom& d) {
    auto up = [](size_t n) { return (n + 15) / 16 * 16; };
    DeflScratch s;
    const size_t nb = (size_t)B, ns = nb * d.nseg;
    s.filt = 0;
    s.hist = s.filt + ns * d.seg_cap;
    s.adl = s.hist + ns * 256 * sizeof(uint32_t);
    s.segbits = s.adl + up(ns * sizeof(uint2));
    s.codes = s.segbits + up((ns + nb) * sizeof(unsigned long long));
    s.meta = s.codes + nb * CODES * sizeof(uint32_t);
    s.bytes = s.meta + nb * 4 * sizeof(uint32_t);
    return s;
}

__device__ inline uint32_t byte_of(const uint32_t (&w)[8], int n) { return (w[n >> 2] >> (8 * (n & 3))) & 255u; }

// Byte e of a lane's 16 under the five filters.  wc / wu: the quad in front of the lane's and the lane's own, of this row and of the row above;
// left: the byte has a pixel to its left
template <int BPP>
__device__ inline void candidates(const uint32_t (&wc)[8], const uint32_t (&wu)[8], int e, bool left, uint32_t (&f)[5]) {
    const int x = byte_of(wc, 16 + e), a = left ? byte_of(wc, 16 + e - BPP) : 0, b = byte_of(wu, 16 + e), c = left ? byte_of(wu, 16 + e - BPP) : 0;
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x, f[1] = (x - a) & 255, f[2] = (x - b) & 255, f[3] = (x - ((a + b) >> 1)) & 255, f[4] = (x - pr) & 255;
}

// filt: the filtered bytes of segment s of image b at (b * nseg + s) * seg_cap; hist[(b * nseg + s) * 256 + v]; adl[b * nseg + s] = (a, b) mod 65521
template <int FMT>
__global__ void __launch_bounds__(PT)
png_filter_kernel(const void* __restrict__ src, int filter, uint8_t* __restrict__ filt, uint32_t* __restrict__ hist, uint2* __restrict__ adl, DeflGeom d) {
    constexpr int BPP = FMT == VIDC_PNG_DEPTH16_F32 ? 2 : FMT == VIDC_PNG_GRAY8_U8 ? 1 : 3;
    __shared__ uint4 cur4[PT + 1], up4[PT + 1];        // raw bytes [lo - 16, lo + 4096) of the chunk at lo, and the bytes one row above them
    __shared__ uint32_t cost[RMAX * 5];
    __shared__ uint32_t h[256];
    __shared__ uint32_t sel[RMAX];
    __shared__ uint32_t red[2][PT / 64];
    const PngGeom& g = d.g;
    const uint32_t t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const size_t HW = (size_t)g.H * g.W;
    const void* img = FMT == VIDC_PNG_GRAY8_U8 ? static_cast<const void*>(static_cast<const uint8_t*>(src) + b * HW)
                                               : static_cast<const void*>(static_cast<const float*>(src) + b * HW * (FMT == VIDC_PNG_DEPTH16_F32 ? 1 : 3));
    const uint32_t r0 = s * d.rps, nrows = min(d.rps, g.H - r0);
    const uint32_t seg_lo = r0 * g.rowbytes, seg_hi = seg_lo + nrows * g.rowbytes, nch = (seg_hi - seg_lo + CH - 1) / CH;
    const bool adaptive = filter == VIDC_PNG_FILTER_ADAPTIVE;
    uint8_t* fseg = filt + ((size_t)b * d.nseg + s) * d.seg_cap;
    for (uint32_t i = t; i < RMAX * 5; i += PT) cost[i] = 0;
    h[t] = 0;
    sel[t] = (uint32_t)filter;

    auto stage = [&](uint32_t lo) {
        uint8_t* cb = reinterpret_cast<uint8_t*>(cur4);
        uint8_t* ub = reinterpret_cast<uint8_t*>(up4);
        for (uint32_t k = t; k < CH + 16; k += PT) {
            const long long i = (long long)lo + k - 16;
            const bool in = i >= 0 && i < (long long)seg_hi;
            cb[k] = in ? (uint8_t)raw_byte<FMT>(img, (uint32_t)i, g, HW) : (uint8_t)0;
            ub[k] = in && i >= (long long)g.rowbytes ? (uint8_t)raw_byte<FMT>(img, (uint32_t)i - g.rowbytes, g, HW) : (uint8_t)0;
        }
    };
    auto quads = [&](uint32_t (&wc)[8], uint32_t (&wu)[8]) {
        const uint4 a = cur4[t], c = cur4[t + 1], ua = up4[t], uc = up4[t + 1];
        wc[0] = a.x, wc[1] = a.y, wc[2] = a.z, wc[3] = a.w, wc[4] = c.x, wc[5] = c.y, wc[6] = c.z, wc[7] = c.w;
        wu[0] = ua.x, wu[1] = ua.y, wu[2] = ua.z, wu[3] = ua.w, wu[4] = uc.x, wu[5] = uc.y, wu[6] = uc.z, wu[7] = uc.w;
    };

    // ---- the five costs of every row
    if (adaptive) {
        for (uint32_t ch = 0; ch < nch; ++ch) {
            const uint32_t lo = seg_lo + ch * CH, hi = min(lo + CH, seg_hi), i0 = lo + 16 * t;
            __syncthreads();
            stage(lo);
            __syncthreads();
            if (i0 < hi) {
                uint32_t wc[8], wu[8], cs[5] = {0, 0, 0, 0, 0};
                quads(wc, wu);
                uint32_t r = i0 / g.rowbytes, c = i0 - r * g.rowbytes;
                auto flush = [&]() {
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        if (cs[k]) atomicAdd(&cost[(r - r0) * 5 + k], cs[k]), cs[k] = 0;
                };
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (i0 + e < hi) {
                        if (c) {
                            uint32_t f[5];
                            candidates<BPP>(wc, wu, e, c > (uint32_t)BPP, f);
#pragma unroll
                            for (int k = 0; k < 5; ++k) cs[k] += f[k] < 128u ? f[k] : 256u - f[k];
                        }
                        if (++c == g.rowbytes) {
                            flush();
                            c = 0, ++r;
                        }
                    }
                }
                flush();
            }
        }
        __syncthreads();
        if (t < nrows) {
            uint32_t best = 0;
#pragma unroll
            for (uint32_t k = 1; k < 5; ++k)
                if (cost[t * 5 + k] < cost[t * 5 + best]) best = k;       // ties: the lowest id
            sel[t] = best;
        }
    }

    // ---- the filtered bytes, their histogram and Adler pair
    unsigned long long A = 0, Bs = 0;        // thread 0: the segment's pair so far
    for (uint32_t ch = 0; ch < nch; ++ch) {
        const uint32_t lo = seg_lo + ch * CH, hi = min(lo + CH, seg_hi), i0 = lo + 16 * t;
        if (!(adaptive && nch == 1)) {       // one chunk: what the cost pass staged is still there
            __syncthreads();
            stage(lo);
        }
        __syncthreads();
        uint32_t al = 0, bl = 0;
        if (i0 < hi) {
            uint32_t wc[8], wu[8], o[4] = {0, 0, 0, 0};
            quads(wc, wu);
            uint32_t r = i0 / g.rowbytes, c = i0 - r * g.rowbytes, fs = sel[r - r0];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (i0 + e < hi) {
                    uint32_t v = fs;
                    if (c) {
                        uint32_t f[5];
                        candidates<BPP>(wc, wu, e, c > (uint32_t)BPP, f);
                        v = fs == 0 ? f[0] : fs == 1 ? f[1] : fs == 2 ? f[2] : fs == 3 ? f[3] : f[4];
                    }
                    o[e >> 2] |= v << (8 * (e & 3));
                    atomicAdd(&h[v], 1u);
                    al += v, bl += al;
                    if (++c == g.rowbytes) {
                        c = 0, ++r;
                        if (r - r0 < nrows) fs = sel[r - r0];
                    }
                }
            }
            *reinterpret_cast<uint4*>(fseg + (i0 - seg_lo)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        // b counts every byte once for itself and once for every byte behind it in the chunk: < 2^32 for 4096 bytes
        const uint32_t behind = i0 < hi ? hi - min(hi, i0 + 16) : 0;
        const uint32_t a_w = wave_add(al), b_w = wave_add(bl + al * behind);
        if ((t & 63) == 0) red[0][t >> 6] = a_w, red[1][t >> 6] = b_w;
        __syncthreads();
        if (t == 0) {
            const unsigned long long a_c = red[0][0] + red[0][1] + red[0][2] + red[0][3];
            const unsigned long long b_c = (unsigned long long)red[1][0] + red[1][1] + red[1][2] + red[1][3];
            A = (A + a_c) % ADLER;
            Bs = (Bs + b_c + a_c * (seg_hi - hi)) % ADLER;
        }
    }
    __syncthreads();
    hist[((size_t)b * d.nseg + s) * 256 + t] = h[t];
    if (t == 0) adl[(size_t)b * d.nseg + s] = make_uint2((uint32_t)A, (uint32_t)Bs);
}

// word w of the 74 bits in front of the lengths: BFINAL 1, BTYPE 10, HLIT 0, HDIST 0, HCLEN 15, then the 19 code-length-code lengths in
// the permuted order: 0 for 16, 17, 18 and 4 for each of 0..15
constexpr uint32_t header_prefix(int w) {
    uint32_t v = 0;
    for (int bit = 32 * w; bit < 32 * w + 32 && bit < (int)HDRLENS; ++bit) {
        bool on = bit == 0 || bit == 2 || (bit >= 13 && bit < 17);
        if (bit >= 17 + 3 * 3 && (bit - 17) % 3 == 2) on = true;
        if (on) v |= 1u << (bit - 32 * w);
    }
    return v;
}

// segbits[b * (nseg + 1) + s]: the file bit at which segment s starts ([nseg]: end-of-block); codes[b * CODES + v] = reversed code | length << 16;
// meta[4 b] = Adler-32, [4 b + 1] = the zlib stream's bytes
__global__ void __launch_bounds__(PT)
png_build_kernel(const uint32_t* __restrict__ hist, const uint2* __restrict__ adl, unsigned long long* __restrict__ segbits, uint32_t* __restrict__ codes,
                 uint32_t* __restrict__ meta, uint8_t* __restrict__ files, size_t file_stride, uint32_t* __restrict__ file_bytes, DeflGeom d) {
    __shared__ uint32_t cnt[NSYM], rnk[NSYM], wsort[NSYM], A[NSYM], len[NSYM];
    __shared__ uint32_t blc[MAXBITS + 1], nxt[MAXBITS + 1];
    __shared__ uint32_t hb[(HDRBITS + 31) / 32 + 1];
    __shared__ uint8_t out[BODY0];
    __shared__ unsigned long long red64[2][PT / 64];
    __shared__ unsigned long long sb[PT];
    const PngGeom& g = d.g;
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const size_t seg0 = (size_t)b * d.nseg;
    // ---- the image's histogram; the Adler sum from the segments' pairs
    {
        uint32_t c = 0;
        for (uint32_t s = 0; s < d.nseg; ++s) c += hist[(seg0 + s) * 256 + t];
        cnt[t] = c;
        if (t == 0) cnt[256] = 1;
        unsigned long long a = 0, bb = 0;
        for (uint32_t s = t; s < d.nseg; s += PT) {
            const uint2 v = adl[seg0 + s];
            const uint32_t seg_hi = min(g.H, (s + 1) * d.rps) * g.rowbytes;
            a += v.x;
            bb += (v.y + (unsigned long long)v.x * (g.raw - seg_hi)) % ADLER;
        }
        a = wave_add(a), bb = wave_add(bb);
        if ((t & 63) == 0) red64[0][t >> 6] = a, red64[1][t >> 6] = bb;
    }
    for (uint32_t i = t; i < sizeof(hb) / 4; i += PT) hb[i] = i < 3 ? header_prefix((int)i) : 0;
    const uint32_t n = (uint32_t)__syncthreads_count(cnt[t] != 0) + 1;       // used symbols: >= 2
    // ---- rank of every used symbol by (count, symbol)
    for (uint32_t v = t; v < NSYM; v += PT) {
        const uint32_t my = cnt[v];
        uint32_t r = 0;
        if (my) {
            for (uint32_t j = 0; j < NSYM; ++j) {
                const uint32_t cj = cnt[j];
                r += cj != 0 && (cj < my || (cj == my && j < v));
            }
            wsort[r] = A[r] = my;
        }
        rnk[v] = r;
    }
    __syncthreads();
    // ---- how many codes of every length
    if (t == 0) {
        for (uint32_t i = 0; i <= MAXBITS; ++i) blc[i] = 0;
        // Moffat and Katajainen, in place on the ascending counts: sums with parent links, then internal depths, then the leaves per depth
        A[0] += A[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next + 1 < n; ++next) {
            if (leaf >= n || A[root] < A[leaf]) A[next] = A[root], A[root++] = next;
            else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = next;
            else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (int next = (int)n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, r = (int)n - 2;
        for (uint32_t dpth = 0; avbl > 0; ++dpth) {
            while (r >= 0 && A[r] == dpth) ++used, --r;
            blc[min(dpth, MAXBITS)] += (uint32_t)(avbl - used);
            avbl = 2 * used, used = 0;
        }
        // deeper than 15: every step moves one leaf one level down and lifts one of the clipped leaves beside it (zlib's gen_bitlen)
        uint32_t kraft = 0;
        for (uint32_t i = 1; i <= MAXBITS; ++i) kraft += blc[i] << (MAXBITS - i);
        for (uint32_t over = kraft - (1u << MAXBITS); over; --over) {
            uint32_t bits = MAXBITS - 1;
            while (blc[bits] == 0) --bits;
            --blc[bits], blc[bits + 1] += 2, --blc[MAXBITS];
        }
        if (kraft != 1u << MAXBITS) {
            // never above the flat code of k = ceil(log2 n) bits: else the balanced code, 2^k - n of length k - 1 and the rest of length k
            unsigned long long cost = 0;
            uint32_t k = 0, bits = MAXBITS, left = blc[MAXBITS];
            for (uint32_t i = 0; i < n; ++i) {
                while (left == 0) left = blc[--bits];
                cost += (unsigned long long)wsort[i] * bits, --left;
            }
            while ((1u << k) < n) ++k;
            if (cost > (unsigned long long)k * (g.raw + 1)) {
                for (uint32_t i = 0; i <= MAXBITS; ++i) blc[i] = 0;
                blc[k - 1] = (1u << k) - n, blc[k] += n - blc[k - 1];
            }
        }
        uint32_t code = 0;
        nxt[0] = 0;
        for (uint32_t bits = 1; bits <= MAXBITS; ++bits) nxt[bits] = code = (code + (bits > 1 ? blc[bits - 1] : 0)) << 1;
    }
    __syncthreads();
    // ---- lengths: the longest to the rarest
    for (uint32_t v = t; v < NSYM; v += PT) {
        uint32_t l = 0;
        if (cnt[v]) {
            uint32_t acc = 0;
            for (l = MAXBITS; acc + blc[l] <= rnk[v]; --l) acc += blc[l];
        }
        len[v] = l;
    }
    __syncthreads();
    // ---- canonical codes (RFC 1951 3.2.2), bit-reversed for the packer; the lengths into the header, each as its own 4-bit code MSB first
    for (uint32_t v = t; v < NSYM + 1; v += PT) {
        const uint32_t l = v < NSYM ? len[v] : 0;        // v = 257: the one distance code, unused
        if (l) {
            uint32_t idx = 0;
            for (uint32_t j = 0; j < v; ++j) idx += len[j] == l;
            codes[(size_t)b * CODES + v] = (__brev(nxt[l] + idx) >> (32 - l)) | l << 16;
            const uint32_t bit = HDRLENS + 4 * v;
            const unsigned long long f = (unsigned long long)(__brev(l) >> 28) << (bit & 31);
            atomicOr(&hb[bit >> 5], (uint32_t)f);
            if (f >> 32) atomicOr(&hb[(bit >> 5) + 1], (uint32_t)(f >> 32));
        } else if (v < NSYM) {
            codes[(size_t)b * CODES + v] = 0;
        }
    }
    __syncthreads();
    // ---- the segments' symbol bits, one wave per segment, 256 segments at a time; their offsets by a scan in LDS
    unsigned long long at = 8ull * BODY0 + HDRBITS;
    for (uint32_t base = 0; base < d.nseg; base += PT) {
        const uint32_t m = min((uint32_t)PT, d.nseg - base);
        for (uint32_t j = t >> 6; j < m; j += PT / 64) {
            unsigned long long bits = 0;
            for (uint32_t v = t & 63; v < 256; v += 64) bits += (unsigned long long)hist[(seg0 + base + j) * 256 + v] * len[v];
            bits = wave_add(bits);
            if ((t & 63) == 0) sb[j] = bits;
        }
        __syncthreads();
        unsigned long long pre = 0, tot = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const unsigned long long v = sb[j];
            pre += j < t ? v : 0ull, tot += v;
        }
        if (t < m) segbits[seg0 + b + base + t] = at + pre;
        at += tot;
        __syncthreads();
    }
    if (t == 0) {
        segbits[seg0 + b + d.nseg] = at;
        const unsigned long long total_bits = at - 8ull * BODY0 + len[256];
        const uint32_t zlen = 2 + (uint32_t)((total_bits + 7) / 8) + 4;
        const unsigned long long a = (1 + red64[0][0] + red64[0][1] + red64[0][2] + red64[0][3]) % ADLER;
        const unsigned long long bb = (g.raw + red64[1][0] + red64[1][1] + red64[1][2] + red64[1][3]) % ADLER;
        meta[4 * b] = (uint32_t)bb << 16 | (uint32_t)a, meta[4 * b + 1] = zlen;
        file_bytes[b] = 57 + zlen;
        png_head(out, g, zlen);
    }
    __syncthreads();
    // ---- the bytes in front of the one that holds the first symbol (its two header bits are zero: the unused distance code's length)
    uint8_t* file = files + b * file_stride;
    if (t < BODY0) file[t] = out[t];
    else if (t < BODY0 + HDRBITS / 8) file[t] = (uint8_t)(hb[(t - BODY0) >> 2] >> (8 * ((t - BODY0) & 3)));
}

__global__ void __launch_bounds__(PT)
png_pack_kernel(const uint8_t* __restrict__ filt, const uint32_t* __restrict__ codes, const unsigned long long* __restrict__ segbits,
                const uint32_t* __restrict__ meta, uint8_t* __restrict__ files, size_t file_stride, DeflGeom d) {
    __shared__ uint32_t tab[NSYM];
    __shared__ uint32_t buf[BUFW];             // the file dwords from the one that holds the chunk's first bit
    __shared__ uint32_t wtot[PT / 64];
    __shared__ uint32_t carry;                 // the bits in front of the chunk in its first dword
    const PngGeom& g = d.g;
    const uint32_t t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const uint32_t nrows = min(d.rps, g.H - s * d.rps), n = nrows * g.rowbytes, nch = (n + CH - 1) / CH;
    const bool last = s + 1 == d.nseg;
    const uint8_t* fseg = filt + ((size_t)b * d.nseg + s) * d.seg_cap;
    uint8_t* file = files + b * file_stride;
    for (uint32_t v = t; v < NSYM; v += PT) tab[v] = codes[(size_t)b * CODES + v];
    unsigned long long P = segbits[(size_t)b * (d.nseg + 1) + s];
    const uint32_t byte_lo = (uint32_t)(P >> 3);
    __syncthreads();
    if (t == 0) {
        // the bits of byte_lo in front of P: zero header bits for segment 0, else the end of the symbols in front (every segment but the last holds >= 8)
        const uint32_t need = (uint32_t)P & 7u;
        uint32_t acc = 0, nacc = 0;
        if (s > 0)
            for (uint32_t k = 1; nacc < need; ++k) {
                const uint32_t e = tab[fseg[(ptrdiff_t)d.rps * g.rowbytes - (ptrdiff_t)d.seg_cap - (ptrdiff_t)k]];
                acc = (e & 0xFFFFu) | acc << (e >> 16), nacc += e >> 16;
            }
        carry = (nacc ? acc >> (nacc - need) : 0u) << (8 * (byte_lo & 3u));
    }
    for (uint32_t ch = 0; ch < nch; ++ch) {
        const uint32_t off = ch * CH + 16 * t, nv = off < n ? min(16u, n - off) : 0u;
        const bool fin = ch + 1 == nch;
        for (uint32_t k = t; k < BUFW; k += PT) buf[k] = 0;
        uint32_t w[4] = {0, 0, 0, 0}, L = 0;
        if (nv) {
            const uint4 q = *reinterpret_cast<const uint4*>(fseg + off);
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if ((uint32_t)e < nv) L += tab[(w[e >> 2] >> (8 * (e & 3))) & 255u] >> 16;
        uint32_t incl = L;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
            if ((int)(t & 63) >= o) incl += up;
        }
        if ((t & 63) == 63) wtot[t >> 6] = incl;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < PT / 64; ++k) base += k < (t >> 6) ? wtot[k] : 0u, total += wtot[k];
        const uint32_t D0 = (uint32_t)(P >> 5);
        {
            const uint32_t pos = ((uint32_t)P & 31u) + base + incl - L;
            uint32_t wi = pos >> 5, nb = pos & 31u;
            unsigned long long acc = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if ((uint32_t)e < nv) {
                    const uint32_t c = tab[(w[e >> 2] >> (8 * (e & 3))) & 255u];
                    acc |= (unsigned long long)(c & 0xFFFFu) << nb;
                    nb += c >> 16;
                    if (nb >= 32) atomicOr(&buf[wi++], (uint32_t)acc), acc >>= 32, nb -= 32;
                }
            if (nb) atomicOr(&buf[wi], (uint32_t)acc);
        }
        if (t == 0) atomicOr(&buf[0], carry);
        __syncthreads();
        const unsigned long long Pend = P + total;
        uint32_t own_hi = 4 * (uint32_t)(Pend >> 5);                 // whole dwords; the rest is the next chunk's carry
        if (fin) own_hi = (uint32_t)(Pend >> 3);                   // whole bytes; the rest belongs to the next segment
        if (fin && last) {
            const uint32_t eob = tab[256], end = (uint32_t)((Pend + (eob >> 16) + 7) >> 3);
            own_hi = end + 4;
            if (t == 0) {
                const uint32_t rel = (uint32_t)(Pend - 32ull * D0), adler = meta[4 * b];
                const unsigned long long v = (unsigned long long)(eob & 0xFFFFu) << (rel & 31u);
                buf[rel >> 5] |= (uint32_t)v, buf[(rel >> 5) + 1] |= (uint32_t)(v >> 32);
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint32_t bi = end + i - 4 * D0;
                    buf[bi >> 2] |= ((adler >> (24 - 8 * i)) & 255u) << (8 * (bi & 3u));
                }
            }
            __syncthreads();
        }
        const uint32_t own_lo = ch == 0 ? byte_lo : 4 * D0;
        for (uint32_t k = t; 4 * (D0 + k) < own_hi; k += PT) {
            const uint32_t fd = 4 * (D0 + k), v = buf[k];
            if (fd >= own_lo && fd + 4 <= own_hi) {
                *reinterpret_cast<uint32_t*>(file + fd) = v;
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e)
                    if (fd + e >= own_lo && fd + e < own_hi) file[fd + e] = (uint8_t)(v >> (8 * e));
            }
        }
        if (!fin && t == 0) carry = buf[(uint32_t)(Pend >> 5) - D0];
        P = Pend;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PT)
png_deflate_close_kernel(const uint32_t* __restrict__ meta, uint8_t* __restrict__ files, size_t file_stride) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t red[PT / 64];
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    uint8_t* file = files + b * file_stride;
    const uint32_t C0 = BODY0 - 6, E = C0 + 4 + meta[4 * b + 1];          // the IDAT type .. the end of the data: what the CRC covers
    {
        uint32_t c = t;
#pragma unroll
        for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (POLY & (0u - (c & 1u)));
        tab[t] = c;
    }
    __syncthreads();
    // lane t: the register from 0 over its 16-byte slices, which lie 4096 bytes apart; then over the bytes behind its last one
    const uint32_t gap = xpow8(SEG - 16);
    uint32_t acc = 0, end = 0;
    for (uint32_t f0 = SEG0 + 16 * t; f0 < E; f0 += SEG) {
        const uint4 q = *reinterpret_cast<const uint4*>(file + f0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        if (end) acc = mulmod(acc, gap);
#pragma unroll
        for (uint32_t e = 0; e < 16; ++e)
            if (f0 + e >= C0 && f0 + e < E) acc = tab[(acc ^ (w[e >> 2] >> (8 * (e & 3)))) & 255u] ^ (acc >> 8);
        end = min(f0 + 16, E);
    }
    uint32_t p = wave_xor(end ? mulmod(acc, xpow8(E - end)) : 0u);
    if ((t & 63) == 0) red[t >> 6] = p;
    __syncthreads();
    if (t < 16) {
        const uint32_t c = ~(mulmod(0xFFFFFFFFu, xpow8(E - C0)) ^ red[0] ^ red[1] ^ red[2] ^ red[3]);
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        file[E + t] = t < 4 ? (uint8_t)(c >> (24 - 8 * t)) : iend[t - 4];
    }
}

}  // namespace

extern "C" size_t vidc_png_deflate_max_file_bytes(int H, int W, int format) {
    DeflGeom d;
    return defl_geom(H, W, format, d) ? (size_t)(57 + d.max_zlib) : 0;
}

extern "C" size_t vidc_png_deflate_scratch_bytes(int B, int H, int W, int format) {
    DeflGeom d;
    return B > 0 && defl_geom(H, W, format, d) ? defl_scratch(B, d).bytes : 0;
}

extern "C" int vidc_png_encode_deflate(const void* src, int B, int H, int W, int format, int filter, uint8_t* files, size_t file_stride,
                                       uint32_t* file_bytes, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(src && files && file_bytes && scratch, VIDC_ERR_NULL, "vidc_png_encode_deflate: null pointer");
    VIDC_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, VIDC_ERR_SHAPE, "vidc_png_encode_deflate: bad shape B=%d H=%d W=%d", B, H, W);
    VIDC_REQUIRE(format >= VIDC_PNG_DEPTH16_F32 && format <= VIDC_PNG_GRAY8_U8, VIDC_ERR_SHAPE, "vidc_png_encode_deflate: unknown format %d", format);
    VIDC_REQUIRE(filter >= VIDC_PNG_FILTER_NONE && filter <= VIDC_PNG_FILTER_ADAPTIVE, VIDC_ERR_SHAPE, "vidc_png_encode_deflate: unknown filter mode %d", filter);
    DeflGeom d;
    VIDC_REQUIRE(defl_geom(H, W, format, d), VIDC_ERR_SHAPE, "vidc_png_encode_deflate: a %dx%d image does not fit one IDAT chunk (2^31 - 1 bytes)", H, W);
    const size_t max_file = (size_t)(57 + d.max_zlib);
    VIDC_REQUIRE(file_stride >= max_file && file_stride % 16 == 0 && reinterpret_cast<uintptr_t>(files) % 16 == 0, VIDC_ERR_SHAPE,
                 "vidc_png_encode_deflate: file_stride %zu must be a multiple of 16 and at least the %zu bytes a file can take, files 16-byte aligned",
                 file_stride, max_file);
    VIDC_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, VIDC_ERR_SHAPE, "vidc_png_encode_deflate: scratch must be 16-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    const DeflScratch sc = defl_scratch(B, d);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint8_t* filt = base + sc.filt;
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + sc.hist);
    uint2* adl = reinterpret_cast<uint2*>(base + sc.adl);
    unsigned long long* segbits = reinterpret_cast<unsigned long long*>(base + sc.segbits);
    uint32_t* codes = reinterpret_cast<uint32_t*>(base + sc.codes);
    uint32_t* meta = reinterpret_cast<uint32_t*>(base + sc.meta);
    const dim3 grid(d.nseg, B);
    switch (format) {
        case VIDC_PNG_DEPTH16_F32: hipLaunchKernelGGL(png_filter_kernel<VIDC_PNG_DEPTH16_F32>, grid, dim3(PT), 0, st, src, filter, filt, hist, adl, d); break;
        case VIDC_PNG_NORMAL8_F32: hipLaunchKernelGGL(png_filter_kernel<VIDC_PNG_NORMAL8_F32>, grid, dim3(PT), 0, st, src, filter, filt, hist, adl, d); break;
        case VIDC_PNG_RGB8_F32: hipLaunchKernelGGL(png_filter_kernel<VIDC_PNG_RGB8_F32>, grid, dim3(PT), 0, st, src, filter, filt, hist, adl, d); break;
        default: hipLaunchKernelGGL(png_filter_kernel<VIDC_PNG_GRAY8_U8>, grid, dim3(PT), 0, st, src, filter, filt, hist, adl, d); break;
    }
    VIDC_CHECK_LAUNCH("png_filter_kernel");
    hipLaunchKernelGGL(png_build_kernel, dim3(B), dim3(PT), 0, st, hist, adl, segbits, codes, meta, files, file_stride, file_bytes, d);
    VIDC_CHECK_LAUNCH("png_build_kernel");
    hipLaunchKernelGGL(png_pack_kernel, grid, dim3(PT), 0, st, filt, codes, segbits, meta, files, file_stride, d);
    VIDC_CHECK_LAUNCH("png_pack_kernel");
    hipLaunchKernelGGL(png_deflate_close_kernel, dim3(B), dim3(PT), 0, st, meta, files, file_stride);
    VIDC_CHECK_LAUNCH("png_deflate_close_kernel");
    return VIDC_OK;
}
