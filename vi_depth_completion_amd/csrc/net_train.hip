// Training ModifiedFPN and SurfaceNormalPrediction under autograd: what torch.ops.vidc needs beyond csrc/train.hip, csrc/sn_train.hip and
// csrc/dorn_train.hip (include/vidc.h, "Training ModifiedFPN and SurfaceNormalPrediction under autograd").  The depth half of `_network_loss`
// (network_run.py:165-179) in one pass: the masked L1 loss with its gradient, the number of valid pixels and the five counts behind
// GetDepthPrintableRatios (network_run.py:72-82).  Every sum: fp64 partials per chunk, reduced in a fixed order by one workgroup -- no atomics,
// no host read, the same bits on every run and stream.
#include "common.h"
#include <cstdint>

namespace {

using vidc::TT;
using vidc::block_tree;

constexpr int kPer = 4;                        // pixels per thread: a chunk is TT * kPer = 1024 pixels
constexpr int kSums = 7;                       // loss, count, ratios[5]
constexpr int kRatios = 5;

inline int loss_chunks(long long n) { return (int)((n + (long long)TT * kPer - 1) / ((long long)TT * kPer)); }

struct Thresholds { float t[kRatios]; };       // the Python scalars 1.05, 1.10, 1.25, 1.25^2, 1.25^3 rounded to fp32, as torch compares an fp32 tensor with them

// partial[blockIdx][kSums] = this chunk's sums.  term and dpred are vidc_masked_l1_loss's (csrc/train.hip, l1_loss_kernel): the same fp32 expressions.
__global__ void __launch_bounds__(TT)
depth_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long long n, float inv_hw, Thresholds th, float* __restrict__ dpred,
                  double* __restrict__ partial) {
    __shared__ double red[kSums][TT];
    const long long base = (long long)blockIdx.x * TT * kPer;
    double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const long long i = base + (long long)k * TT + threadIdx.x;
        if (i >= n) continue;
        const float p = pred[i], g = gt[i], d = p - g;
        const bool on = g > 0.f;
        dpred[i] = on ? (d > 0.f ? inv_hw : (d < 0.f ? -inv_hw : 0.f)) : 0.f;
        if (!on) continue;
        s[0] += (double)(fabsf(d) * inv_hw);
        s[1] += 1.0;
        const float r = fmaxf(p / g, g / p);          // IEEE fp32 quotients; p == 0: g / p = inf, counted nowhere; a NaN compares false
#pragma unroll
        for (int j = 0; j < kRatios; ++j) s[2 + j] += r < th.t[j] ? 1.0 : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j) red[j][threadIdx.x] = s[j];
    block_tree<kSums>(red);
    if (threadIdx.x < kSums) partial[(size_t)blockIdx.x * kSums + threadIdx.x] = red[threadIdx.x][0];
}

// One workgroup: the nb partial rows in a fixed order.
__global__ void __launch_bounds__(TT)
depth_loss_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ loss, double* __restrict__ count, double* __restrict__ ratios) {
    __shared__ double red[kSums][TT];
    double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += TT) {
#pragma unroll
        for (int j = 0; j < kSums; ++j) s[j] += partial[(size_t)i * kSums + j];
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j) red[j][threadIdx.x] = s[j];
    block_tree<kSums>(red);
    if (threadIdx.x == 0) {
        *loss = red[0][0];
        *count = red[1][0];
    }
    if (threadIdx.x < kRatios) ratios[threadIdx.x] = red[2 + threadIdx.x][0];
}

}  // namespace

extern "C" size_t vidc_depth_l1_loss_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)loss_chunks((long long)B * H * W) * kSums * sizeof(double);
}

extern "C" int vidc_depth_l1_loss(const float* pred, const float* depth_gt, int B, int H, int W, double* loss, double* count, double* ratios, float* dpred,
                                  void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(pred && depth_gt && loss && count && ratios && dpred && scratch, VIDC_ERR_NULL, "vidc_depth_l1_loss: null pointer");
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0, VIDC_ERR_SHAPE, "vidc_depth_l1_loss: bad shape");
    VIDC_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, VIDC_ERR_SHAPE, "vidc_depth_l1_loss: scratch must be 8-byte aligned");
    const long long hw = (long long)H * W, n = (long long)B * hw;
    VIDC_REQUIRE(hw < (1ll << 31) && (n + (long long)TT * kPer - 1) / ((long long)TT * kPer) < (1ll << 31), VIDC_ERR_SHAPE,
                 "vidc_depth_l1_loss: too many pixels for one launch");
    hipStream_t st = vidc::as_stream(stream);
    const int nb = loss_chunks(n);
    double* partial = reinterpret_cast<double*>(scratch);
    const Thresholds th = {{1.05f, 1.10f, 1.25f, 1.5625f, 1.953125f}};
    hipLaunchKernelGGL(depth_loss_kernel, dim3(nb), dim3(TT), 0, st, pred, depth_gt, n, 1.0f / (float)hw, th, dpred, partial);
    hipLaunchKernelGGL(depth_loss_final_kernel, dim3(1), dim3(TT), 0, st, partial, nb, loss, count, ratios);
    VIDC_CHECK_LAUNCH("depth_l1_loss");
    return VIDC_OK;
}
