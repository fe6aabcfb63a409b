// Training step of the surface-normal network: what it needs beyond csrc/train.hip (include/vidc.h, "Training step of the surface-normal
// network").  The normal loss of network_run.py:181-189 / normal_utils.py:20-34 with its gradient.  Every sum: fp64 partials per workgroup,
// reduced in a fixed order -- no floating-point atomics, the same bits on every run and stream.
#include "common.h"
#include <cstdint>

namespace {

using vidc::TT;
using vidc::blocks;
using vidc::block_tree;
constexpr double kNormEps = 1e-12;            // F.normalize's default eps
constexpr double kDegPerRad = 57.295779513082320876798154814105;

// ---- normal loss ---------------------------------------------------------------------------------------------------------------------
// One pixel: n = pred (or F.normalize(pred)), gh = F.normalize(gt), m = mask > 0.  term = m * sum_c |n_c - gh_c|, angle = m * acos(clamp(n . gh))
// in degrees, d = the gradient of `term` w.r.t. pred (NOT yet divided by N = sum m).  fp64 from the fp32 inputs: acos next to +-1 is what fp32
// gets wrong, and the kernel is bound by its memory traffic.
__device__ inline void normal_loss_pixel(float p0, float p1, float p2, float g0, float g1, float g2, float mk, int normalize_prediction, double& term,
                                         double& angle, double& cnt, float& d0, float& d1, float& d2) {
    if (!(mk > 0.f)) {
        d0 = d1 = d2 = 0.f;
        return;
    }
    const double gx = g0, gy = g1, gz = g2;
    const double gi = 1.0 / fmax(sqrt(gx * gx + gy * gy + gz * gz), kNormEps);
    const double hx = gx * gi, hy = gy * gi, hz = gz * gi;
    double nx = p0, ny = p1, nz = p2, nrm = 0.0;
    if (normalize_prediction) {
        nrm = sqrt(nx * nx + ny * ny + nz * nz);
        const double ni = 1.0 / fmax(nrm, kNormEps);
        nx *= ni; ny *= ni; nz *= ni;
    }
    const double ex = nx - hx, ey = ny - hy, ez = nz - hz;
    term += fabs(ex) + fabs(ey) + fabs(ez);
    const double dot = fmin(fmax(nx * hx + ny * hy + nz * hz, -1.0), 1.0);
    angle += acos(dot) * kDegPerRad;
    cnt += 1.0;
    double sx = ex > 0.0 ? 1.0 : (ex < 0.0 ? -1.0 : 0.0);      // sign(0) = 0, torch's L1 backward
    double sy = ey > 0.0 ? 1.0 : (ey < 0.0 ? -1.0 : 0.0);
    double sz = ez > 0.0 ? 1.0 : (ez < 0.0 ? -1.0 : 0.0);
    if (normalize_prediction) {
        if (nrm >= kNormEps) {                                  // d(x / |x|): (s - n (n . s)) / |x|
            const double ns = nx * sx + ny * sy + nz * sz, ri = 1.0 / nrm;
            sx = (sx - nx * ns) * ri; sy = (sy - ny * ns) * ri; sz = (sz - nz * ns) * ri;
        } else {                                                // the clamp holds the denominator at eps and passes no gradient
            sx *= 1.0 / kNormEps; sy *= 1.0 / kNormEps; sz *= 1.0 / kNormEps;
        }
    }
    d0 = (float)sx; d1 = (float)sy; d2 = (float)sz;
}

// V pixels per thread (V = 4: 16-byte loads and stores, HW % 4 == 0 so that a thread's pixels share an image).  partial[blockIdx][3] = this
// workgroup's sums of (term, count, angle).
template <int V>
__global__ void __launch_bounds__(TT)
normal_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask, long long n_pix, int HW,
                   int normalize_prediction, float* __restrict__ dpred, double* __restrict__ partial) {
    __shared__ double red[3][TT];
    const long long q = ((long long)blockIdx.x * TT + threadIdx.x) * V;
    double term = 0.0, angle = 0.0, cnt = 0.0;
    if (q < n_pix) {
        const long long b = q / HW;
        const long long o = b * 3 * HW + (q - b * HW);          // channel 0 of pixel q; channels are HW apart
        if constexpr (V == 4) {
            const float4 p0 = *reinterpret_cast<const float4*>(pred + o), p1 = *reinterpret_cast<const float4*>(pred + o + HW),
                         p2 = *reinterpret_cast<const float4*>(pred + o + 2ll * HW);
            const float4 g0 = *reinterpret_cast<const float4*>(gt + o), g1 = *reinterpret_cast<const float4*>(gt + o + HW),
                         g2 = *reinterpret_cast<const float4*>(gt + o + 2ll * HW);
            const float4 mk = *reinterpret_cast<const float4*>(mask + q);
            float4 d0, d1, d2;
            normal_loss_pixel(p0.x, p1.x, p2.x, g0.x, g1.x, g2.x, mk.x, normalize_prediction, term, angle, cnt, d0.x, d1.x, d2.x);
            normal_loss_pixel(p0.y, p1.y, p2.y, g0.y, g1.y, g2.y, mk.y, normalize_prediction, term, angle, cnt, d0.y, d1.y, d2.y);
            normal_loss_pixel(p0.z, p1.z, p2.z, g0.z, g1.z, g2.z, mk.z, normalize_prediction, term, angle, cnt, d0.z, d1.z, d2.z);
            normal_loss_pixel(p0.w, p1.w, p2.w, g0.w, g1.w, g2.w, mk.w, normalize_prediction, term, angle, cnt, d0.w, d1.w, d2.w);
            *reinterpret_cast<float4*>(dpred + o) = d0;
            *reinterpret_cast<float4*>(dpred + o + HW) = d1;
            *reinterpret_cast<float4*>(dpred + o + 2ll * HW) = d2;
        } else {
            float d0, d1, d2;
            normal_loss_pixel(pred[o], pred[o + HW], pred[o + 2ll * HW], gt[o], gt[o + HW], gt[o + 2ll * HW], mask[q], normalize_prediction, term, angle, cnt,
                              d0, d1, d2);
            dpred[o] = d0; dpred[o + HW] = d1; dpred[o + 2ll * HW] = d2;
        }
    }
    red[0][threadIdx.x] = term; red[1][threadIdx.x] = cnt; red[2][threadIdx.x] = angle;
    block_tree<3>(red);
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * 3 + 0] = red[0][0];
        partial[(size_t)blockIdx.x * 3 + 1] = red[1][0];
        partial[(size_t)blockIdx.x * 3 + 2] = red[2][0];
    }
}

// One workgroup: the nb partial triples in a fixed order; loss = sum / N, and 1 / N left in device memory for the scale pass.
__global__ void __launch_bounds__(TT)
normal_loss_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ loss, double* __restrict__ count, double* __restrict__ angle,
                         double* __restrict__ inv_count) {
    __shared__ double red[3][TT];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nb; i += TT) {
        s0 += partial[(size_t)i * 3 + 0];
        s1 += partial[(size_t)i * 3 + 1];
        s2 += partial[(size_t)i * 3 + 2];
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    block_tree<3>(red);
    if (threadIdx.x == 0) {
        const double N = red[1][0];
        *loss = red[0][0] / N;                 // N == 0 divides by zero, as the reference does
        if (count) *count = N;
        if (angle) *angle = red[2][0];
        *inv_count = 1.0 / N;
    }
}

template <int V>
__global__ void __launch_bounds__(TT) normal_loss_scale_kernel(float* __restrict__ dpred, long long n, const double* __restrict__ inv_count) {
    const long long i = ((long long)blockIdx.x * TT + threadIdx.x) * V;
    if (i >= n) return;
    const double s = *inv_count;
    if constexpr (V == 4) {
        float4 d = *reinterpret_cast<float4*>(dpred + i);
        d.x = (float)(d.x * s); d.y = (float)(d.y * s); d.z = (float)(d.z * s); d.w = (float)(d.w * s);
        *reinterpret_cast<float4*>(dpred + i) = d;
    } else {
        dpred[i] = (float)(dpred[i] * s);
    }
}

inline int normal_loss_blocks(long long n_pix, int V) { return (int)((n_pix + (long long)TT * V - 1) / ((long long)TT * V)); }

}  // namespace

extern "C" size_t vidc_normal_l1_loss_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ((size_t)normal_loss_blocks((long long)B * H * W, 1) * 3 + 8) * sizeof(double);      // (the scalar form has the most workgroups)
}

extern "C" int vidc_normal_l1_loss(const float* pred, const float* normal_gt, const float* mask, int B, int H, int W, int normalize_prediction, double* loss,
                                   double* count, double* angle, float* dpred, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(pred && normal_gt && mask && loss && dpred && scratch, VIDC_ERR_NULL, "vidc_normal_l1_loss: null pointer");
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0, VIDC_ERR_SHAPE, "vidc_normal_l1_loss: bad shape");
    VIDC_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, VIDC_ERR_SHAPE, "vidc_normal_l1_loss: scratch must be 8-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    const long long HW = (long long)H * W, n_pix = (long long)B * HW;
    VIDC_REQUIRE(HW < (1ll << 31), VIDC_ERR_SHAPE, "vidc_normal_l1_loss: one image must have fewer than 2^31 pixels");
    const bool wide = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(normal_gt) | reinterpret_cast<uintptr_t>(mask) |
                                       reinterpret_cast<uintptr_t>(dpred)) & 15) == 0;
    double* inv_count = reinterpret_cast<double*>(scratch);
    double* partial = inv_count + 8;
    const int nb = normal_loss_blocks(n_pix, wide ? 4 : 1);
    if (wide)
        hipLaunchKernelGGL(normal_loss_kernel<4>, dim3(nb), dim3(TT), 0, st, pred, normal_gt, mask, n_pix, (int)HW, normalize_prediction, dpred, partial);
    else
        hipLaunchKernelGGL(normal_loss_kernel<1>, dim3(nb), dim3(TT), 0, st, pred, normal_gt, mask, n_pix, (int)HW, normalize_prediction, dpred, partial);
    hipLaunchKernelGGL(normal_loss_final_kernel, dim3(1), dim3(TT), 0, st, partial, nb, loss, count, angle, inv_count);
    const long long n = 3 * n_pix;
    if (wide)
        hipLaunchKernelGGL(normal_loss_scale_kernel<4>, dim3(blocks(n / 4)), dim3(TT), 0, st, dpred, n, inv_count);
    else
        hipLaunchKernelGGL(normal_loss_scale_kernel<1>, dim3(blocks(n)), dim3(TT), 0, st, dpred, n, inv_count);
    VIDC_CHECK_LAUNCH("normal_l1_loss");
    return VIDC_OK;
}
