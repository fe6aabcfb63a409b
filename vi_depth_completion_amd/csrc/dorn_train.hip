// Training SurfaceNormalDORN under autograd: what torch.ops.vidc needs beyond csrc/train.hip and csrc/sn_train.hip (include/vidc.h, "Training
// SurfaceNormalDORN").  nn.Dropout2d as a counter-based keep table plus a per-(image, channel) scale pass, and the adjoint of vidc_normalize_nchw.
// No device state, no host read: every entry is capturable.
#include "common.h"
#include <cstdint>

namespace {

using vidc::TT;
using vidc::blocks;
constexpr double kNormEps = 1e-12;            // F.normalize's default eps

// ---- Philox4x32-10 (Salmon et al., SC'11) ------------------------------------------------------------------------------------------------
// The first output word of the block whose counter is (c0, c1, c2, c3) under the key (k0, k1).
__device__ inline unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// keep[i], i = b * C + c: 0 or 1 / (1 - p).
__global__ void __launch_bounds__(TT) dropout2d_mask_kernel(float* __restrict__ keep, int n, float p, float kept, unsigned seed_lo, unsigned seed_hi,
                                                            unsigned off_lo, unsigned off_hi) {
    const int i = blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const unsigned w = philox4x32_10_word0(off_lo, (unsigned)i, off_hi, 0u, seed_lo, seed_hi);
    const float u = (float)(w >> 8) * 0x1p-24f;          // 24 bits: exact in fp32
    keep[i] = u >= p ? kept : 0.f;
}

// y[b,h,w,c] = x[b,h,w,c] * k[b][c]: one thread per four channels of one pixel.  y may be x.
__global__ void __launch_bounds__(TT) scale_image_channels_kernel(const float* x, const float* __restrict__ k, float* y, long long n4, int HW, int C, int ldx,
                                                                  int ldy) {
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    if (i >= n4) return;
    const int c4 = C / 4;
    const long long row = i / c4;
    const int c = (int)(i - row * c4) * 4;
    const long long b = row / HW;
    const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + c);
    const float4 s = *reinterpret_cast<const float4*>(k + b * C + c);
    *reinterpret_cast<float4*>(y + row * ldy + c) = make_float4(v.x * s.x, v.y * s.y, v.z * s.z, v.w * s.w);
}

// One pixel per thread, channels HW apart.  fp64 from the fp32 inputs, the rule of normal_loss_pixel (csrc/sn_train.hip) for any C:
// (g - n (n . g)) / |x| where |x| >= eps, g / eps below it (the clamp passes no gradient).
__global__ void __launch_bounds__(TT) normalize_nchw_backward_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                                     long long n_pix, int C, int HW) {
    const long long q = (long long)blockIdx.x * TT + threadIdx.x;
    if (q >= n_pix) return;
    const long long b = q / HW;
    const long long o = b * C * HW + (q - b * HW);
    double ss = 0.0, xg = 0.0;
    for (int c = 0; c < C; ++c) {
        const double v = x[o + (long long)c * HW];
        ss += v * v;
        xg += v * (double)dy[o + (long long)c * HW];
    }
    const double nrm = sqrt(ss);
    if (nrm >= kNormEps) {
        const double ri = 1.0 / nrm, ng = xg * ri;           // n . g
        for (int c = 0; c < C; ++c) {
            const double n = x[o + (long long)c * HW] * ri;
            dx[o + (long long)c * HW] = (float)((dy[o + (long long)c * HW] - n * ng) * ri);
        }
    } else {
        for (int c = 0; c < C; ++c) dx[o + (long long)c * HW] = (float)(dy[o + (long long)c * HW] / kNormEps);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int vidc_dropout2d_mask(float* keep, int B, int C, float p, unsigned long long seed, unsigned long long offset, vidc_stream_t stream) {
    VIDC_REQUIRE(keep, VIDC_ERR_NULL, "vidc_dropout2d_mask: null pointer");
    VIDC_REQUIRE(B > 0 && C > 0 && (long long)B * C < (1ll << 31), VIDC_ERR_SHAPE, "vidc_dropout2d_mask: bad shape");
    VIDC_REQUIRE(p >= 0.f && p < 1.f, VIDC_ERR_SHAPE, "vidc_dropout2d_mask: p must be in [0, 1)");
    const int n = B * C;
    hipLaunchKernelGGL(dropout2d_mask_kernel, dim3(blocks(n)), dim3(TT), 0, vidc::as_stream(stream), keep, n, p, 1.0f / (1.0f - p), (unsigned)seed,
                       (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32));
    VIDC_CHECK_LAUNCH("dropout2d_mask_kernel");
    return VIDC_OK;
}

extern "C" int vidc_scale_image_channels(const float* x, const float* k, float* y, int B, int HW, int C, int ldx, int ldy, vidc_stream_t stream) {
    VIDC_REQUIRE(x && k && y, VIDC_ERR_NULL, "vidc_scale_image_channels: null pointer");
    VIDC_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0, VIDC_ERR_SHAPE,
                 "vidc_scale_image_channels: bad shape (C, ldx, ldy multiples of 4; ldx, ldy >= C)");
    VIDC_REQUIRE(aligned16(x) && aligned16(k) && aligned16(y), VIDC_ERR_SHAPE, "vidc_scale_image_channels: x, k and y must be 16-byte aligned");
    const long long n4 = (long long)B * HW * (C / 4);
    VIDC_REQUIRE((n4 + TT - 1) / TT < (1ll << 31), VIDC_ERR_SHAPE, "vidc_scale_image_channels: too many elements for one launch");
    hipLaunchKernelGGL(scale_image_channels_kernel, dim3(blocks(n4)), dim3(TT), 0, vidc::as_stream(stream), x, k, y, n4, HW, C, ldx, ldy);
    VIDC_CHECK_LAUNCH("scale_image_channels_kernel");
    return VIDC_OK;
}

extern "C" int vidc_normalize_nchw_backward(const float* x, const float* dy, float* dx, int B, int C, int HW, vidc_stream_t stream) {
    VIDC_REQUIRE(x && dy && dx, VIDC_ERR_NULL, "vidc_normalize_nchw_backward: null pointer");
    VIDC_REQUIRE(B > 0 && C > 0 && HW > 0, VIDC_ERR_SHAPE, "vidc_normalize_nchw_backward: bad shape");
    const long long n_pix = (long long)B * HW;
    VIDC_REQUIRE((n_pix + TT - 1) / TT < (1ll << 31), VIDC_ERR_SHAPE, "vidc_normalize_nchw_backward: too many pixels for one launch");
    hipLaunchKernelGGL(normalize_nchw_backward_kernel, dim3(blocks(n_pix)), dim3(TT), 0, vidc::as_stream(stream), x, dy, dx, n_pix, C, HW);
    VIDC_CHECK_LAUNCH("normalize_nchw_backward_kernel");
    return VIDC_OK;
}
