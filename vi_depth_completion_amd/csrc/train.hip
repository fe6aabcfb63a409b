// Training step of the depth-completion network on the device: what `_run_training_iteration` (network_run.py:231-254)
// needs beyond the inference kernels -- BatchNorm in train() mode (batch statistics + running-statistic update) and its backward, the
// backward of ReLU / residual add / max-pool / bilinear upsampling / the padded 1x1 head, the weight gradients of the convolutions
// (wgrad: an fp32-MFMA GEMM whose reduction runs over the pixels), the masked L1 loss of `_network_loss` (network_run.py:158-173)
// and torch.optim.Adam's update (network_run.py:228-229).  The data gradients of the convolutions (dgrad) are the forward conv kernel
// (conv_mfma.hip) on flipped / transposed weights (pack_weight_dgrad_kernel here), with stride-2 layers going through a zero-stuffed
// copy of the incoming gradient.
//
// Layout: activations NHWC fp32, `ld` = channel stride of a row (a tensor may be a channel slice of a concat buffer).  Per-channel
// reductions accumulate in fp64 with a fixed two-level order (bit-reproducible), like torch's CPU kernels accumulate float in double.
#include "common.h"
#include "train_rows.h"
#include "optim.h"
#include "wgrad_final.h"
#include <cstdint>
#include <type_traits>

namespace {

using vidc::TT;
using vidc::blocks;
using vidc::block_tree;
using vidc::adam_one;
using vidc::row_quad, vidc::load4, vidc::store4, vidc::store4_bf16, vidc::store8_bf16, vidc::relu_mask4;      // train_rows.h

// What the per-channel sums become, applied by the thread that finishes a channel in chan_final_kernel (no extra launch).
// batch mean, biased variance and invstd from the two per-channel sums (shared by chan_final_kernel's FinalStats and the kernels that
// fold that reduction into their prologue, so that both forms round identically)
struct BnMoments { double mu, var; float mean, rstd; };
__device__ inline BnMoments bn_moments(double s0, double s1, long long M, float eps) {
    BnMoments r;
    r.mu = s0 / (double)M;
    r.var = s1 / (double)M - r.mu * r.mu;
    if (r.var < 0.0) r.var = 0.0;
    r.mean = (float)r.mu;
    r.rstd = (float)(1.0 / sqrt(r.var + (double)eps));
    return r;
}
__device__ inline void bn_update_running(float* running_mean, float* running_var, int c, const BnMoments& m, long long M, float momentum) {
    const double unbiased = M > 1 ? m.var * (double)M / (double)(M - 1) : m.var;
    running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * m.mu);
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
}

struct FinalStats {      // nn.BatchNorm2d.forward in train(): batch mean, biased variance, invstd = 1/sqrt(var + eps); running_mean/var <-
    long long M;         // (1 - momentum) * old + momentum * (mean, unbiased var)
    float eps, momentum;
    float *mean, *rstd, *running_mean, *running_var;
    __device__ void operator()(int c, double s0, double s1) const {
        const BnMoments m = bn_moments(s0, s1, M, eps);
        mean[c] = m.mean;
        rstd[c] = m.rstd;
        if (running_mean) bn_update_running(running_mean, running_var, c, m, M, momentum);
    }
};
struct FinalParamGrad {  // dbeta = sum dy, dgamma = sum dy * xhat
    float *dgamma, *dbeta;
    __device__ void operator()(int c, double s0, double s1) const { dbeta[c] = (float)s0; dgamma[c] = (float)s1; }
};
struct FinalColsum {     // bias gradient of a conv: column sums of dY (first sum only)
    float* out;
    __device__ void operator()(int c, double s0, double) const { out[c] = (float)s0; }
};

// The chunk sums of a 64-channel column added up exactly as chan_final_kernel adds them -- lane j takes chunks j, j + 32, ... in order,
// then the fixed pairwise tree over the 32 lanes -- by the 256 threads of ONE workgroup: thread = channel l x 8 of the 32 lanes, the 16
// loads of a round issued together, the tree through LDS.  Result: red[q][0][l].  Used by the kernels that fold the final reduction into
// their prologue (bn_apply_fold_kernel, bn_bwd_apply_t64_kernel<true>).  Bit-identical to chan_final_kernel.
__device__ __forceinline__ void column_sums(const double* __restrict__ partial, int n_chunks, int C, int c0, double (*red)[32][64]) {
    const int l = threadIdx.x & 63, j0 = (threadIdx.x >> 6) * 8, cc = c0 + l;
    double t0[8], t1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { t0[j] = 0.0; t1[j] = 0.0; }
    if (cc < C)
        for (int k0 = 0; k0 < n_chunks; k0 += 32) {
            double u0[8], u1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = min(k0 + j0 + j, n_chunks - 1);
                const double* src = partial + ((size_t)k * 2) * C + cc;
                u0[j] = src[0];
                u1[j] = src[C];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k0 + j0 + j < n_chunks) { t0[j] += u0[j]; t1[j] += u1[j]; }
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[0][j0 + j][l] = t0[j]; red[1][j0 + j][l] = t1[j]; }
    __syncthreads();
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {            // chan_final_kernel's tree: lane j += lane j + w for j < w
        for (int i = threadIdx.x; i < w * 64; i += TT) {
            const int j = i >> 6, ll = i & 63;
            red[0][j][ll] += red[0][j + w][ll];
            red[1][j][ll] += red[1][j + w][ll];
        }
        __syncthreads();
    }
}

// ---- BatchNorm on one row quad (train_rows.h): the one forward body and the one backward body of every launch form ------------------
// y = x * alpha + bb with alpha = invstd * gamma, bb = beta - mean * alpha (torch's batch_norm_cpu_transform_input), + res (the Bottleneck
// tail relu(bn3(.) + identity) in the same pass: the BatchNorm value is rounded to fp32 before the sum, as when a separate add kernel read
// it back), ReLU optional; y_bf16 != NULL: also the bf16 operand copy the next conv of a VIDC_PREC_BF16 step reads (dense rows of C bf16),
// saving its cast launch.  Row r, channels c..c+3 of every tensor; res and y_bf16 may be NULL.
__device__ __forceinline__ void bn_apply_row(long long r, int c, const float* __restrict__ x, int ldx, const float* __restrict__ res, int ldr,
                                             float* __restrict__ y, int ldy, unsigned short* __restrict__ y_bf16, int C, const float* alpha,
                                             const float* bb, int relu) {
    float in[4], out[4], add[4] = {0.f, 0.f, 0.f, 0.f};
    load4(x + r * ldx + c, in);
    if (res) load4(res + r * ldr + c, add);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float o = in[k] * alpha[k] + bb[k];
        if (res) o = __fadd_rn(o, add[k]);
        out[k] = relu ? fmaxf(o, 0.f) : o;
    }
    store4(y + r * ldy + c, out);
    if (y_bf16) store4_bf16(y_bf16 + r * C + c, out);
}
// The operands of the backward: g holds dy on entry and dy' = dy * (y > 0) on return (y != NULL: the output of the ReLU that followed the
// BatchNorm), xh = (x - mean) * invstd.  Shared by the reduction (chan_partial_kernel<1>) and the apply pass (bn_bwd_row).
__device__ __forceinline__ void bn_bwd_operands(float* g, float* xh, long long r, int c, const float* __restrict__ x, int ldx,
                                                const float* __restrict__ y, int ldy, const float* mu, const float* rs) {
    float xv[4];
    load4(x + r * ldx + c, xv);
    if (y) {
        float yv[4];
        load4(y + r * ldy + c, yv);
        relu_mask4(g, yv);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xh[k] = (xv[k] - mu[k]) * rs[k];
}
// dx = gs * (dy' - m1 - xhat * m2) with gs = gamma * invstd, m1 = sum(dy') / M, m2 = sum(dy' * xhat) / M (dgamma = sum(dy' * xhat), dbeta =
// sum(dy')); o -> dx (NULL: nobody reads the fp32 form) and dx_bf16 (dense rows of C bf16; NULL: not wanted), and back to the caller.
__device__ __forceinline__ void bn_bwd_row(long long r, int c, const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                           const float* __restrict__ y, int ldy, float* __restrict__ dx, int lddx, unsigned short* __restrict__ dx_bf16,
                                           int C, const float* mu, const float* rs, const float* gs, const float* m1, const float* m2, float* o) {
    float g[4], xh[4];
    load4(dy + r * lddy + c, g);
    bn_bwd_operands(g, xh, r, c, x, ldx, y, ldy, mu, rs);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = gs[k] * (g[k] - m1[k] - xh[k] * m2[k]);
    if (dx) store4(dx + r * lddx + c, o);
    if (dx_bf16) store4_bf16(dx_bf16 + r * C + c, o);
}

// ---- per-channel sums over rows: partial[chunk][q][C] (fp64) -------------------------------------------------------------------------
// block = 256 threads = 64 channels x 4 row-lanes; grid = (C/64 rounded up, n_chunks).  MODE 0: sum x, sum x^2.  MODE 1 (BN backward):
// sum dy', sum dy' * xhat with dy' = dy * (y > 0) when y != NULL (the ReLU that followed the BatchNorm).
template <int MODE>
__global__ void __launch_bounds__(TT)
chan_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ y, long long M, int C, int lda, int ldb,
                    int ldy, const float* __restrict__ mean, const float* __restrict__ rstd, int rows_per_chunk, double* __restrict__ partial) {
    // block = 16 channel quads (64 channels, one float4 per thread and row) x 16 row-lanes; C % 4 == 0 and the strides % 4 == 0 (host-checked)
    __shared__ double red[2][16][64];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    if (c < C) {
        float mu[4] = {0, 0, 0, 0}, rs[4] = {0, 0, 0, 0};
        if (MODE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { mu[k] = mean[c + k]; rs[k] = rstd[c + k]; }
        }
        for (long long r = r0 + rl; r < r1; r += 16) {
            float g[4];
            load4(a + r * lda + c, g);
            if (MODE == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double v = (double)g[k]; s0[k] += v; s1[k] += v * v; }
            } else {
                float xh[4];
                bn_bwd_operands(g, xh, r, c, b, ldb, y, ldy, mu, rs);
#pragma unroll
                for (int k = 0; k < 4; ++k) { s0[k] += (double)g[k]; s1[k] += (double)g[k] * (double)xh[k]; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[0][rl][cq * 4 + k] = s0[k]; red[1][rl][cq * 4 + k] = s1[k]; }
    __syncthreads();
    if (threadIdx.x < 128) {                       // 64 channels x 2 sums; row-lanes added in order 0..15
        const int q = threadIdx.x >> 6, l = threadIdx.x & 63, cc = blockIdx.x * 64 + l;
        if (cc < C) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) t += red[q][j][l];
            partial[((size_t)blockIdx.y * 2 + q) * C + cc] = t;
        }
    }
}

// sums[q][C] = sum over chunks: block = 8 channels x 32 lanes; lane l adds chunks l, l+32, ... in order, then the 32 lane sums are added
// pairwise (a fixed tree) -- bit-reproducible; `fin` then turns the two sums of a channel into the op's per-channel outputs
template <typename Final>
__global__ void __launch_bounds__(TT) chan_final_kernel(const double* __restrict__ partial, int n_chunks, int C, double* __restrict__ sums, Final fin) {
    __shared__ double red[2][32][8];
    const int l = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + l;
    double s0 = 0.0, s1 = 0.0;
    if (c < C)
        for (int k = rl; k < n_chunks; k += 32) { s0 += partial[((size_t)k * 2 + 0) * C + c]; s1 += partial[((size_t)k * 2 + 1) * C + c]; }
    red[0][rl][l] = s0; red[1][rl][l] = s1;
    __syncthreads();
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        if (rl < w) { red[0][rl][l] += red[0][rl + w][l]; red[1][rl][l] += red[1][rl + w][l]; }
        __syncthreads();
    }
    if (rl == 0 && c < C) {
        s0 = red[0][0][l];
        s1 = red[1][0][l];
        sums[c] = s0;
        sums[C + c] = s1;
        fin(c, s0, s1);
    }
}

// The kernels below fold the final reduction into their prologue -- every workgroup redoes it for its 64 channels from the L2-resident
// chunk sums (column_sums) -- which removes the chan_final launch between the partial-sum kernel and its consumer without any
// cross-workgroup hand-off.  Bit-identical.
// chan_final<FinalStats> + bn_apply_kernel in one launch: 64 pixels x 64 channels per workgroup (the layout of bn_bwd_apply_t64_kernel).
__global__ void __launch_bounds__(256)
bn_apply_fold_kernel(const float* __restrict__ x, float* __restrict__ y, int M, int C, int ldx, int ldy, const double* __restrict__ partial, int n_chunks,
                     float eps, float momentum, float* __restrict__ save_mean, float* __restrict__ save_rstd, float* __restrict__ running_mean,
                     float* __restrict__ running_var, const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                     unsigned short* __restrict__ y_bf16, const float* __restrict__ res, int ldr) {
    __shared__ double red[2][32][64];
    __shared__ float mean_s[64], rstd_s[64];
    const int c0 = blockIdx.y * 64, m0 = blockIdx.x * 64;
    column_sums(partial, n_chunks, C, c0, red);
    if (threadIdx.x < 64) {
        const int l = threadIdx.x, cc = c0 + l;
        const BnMoments mo = bn_moments(red[0][0][l], red[1][0][l], (long long)M, eps);
        mean_s[l] = mo.mean; rstd_s[l] = mo.rstd;
        if (blockIdx.x == 0 && cc < C) {         // one workgroup per channel block publishes what the backward and the module keep
            save_mean[cc] = mo.mean; save_rstd[cc] = mo.rstd;
            if (running_mean) bn_update_running(running_mean, running_var, cc, mo, (long long)M, momentum);
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int c = c0 + tx * 4;
    if (c >= C) return;
    float alpha[4], bb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        alpha[k] = rstd_s[tx * 4 + k] * gamma[c + k];
        bb[k] = beta[c + k] - mean_s[tx * 4 + k] * alpha[k];
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = m0 + ty + 16 * rr;
        if (r >= M) continue;
        bn_apply_row(r, c, x, ldx, res, ldr, y, ldy, y_bf16, C, alpha, bb, relu);
    }
}

// bn_apply_row on a flat launch, one thread per row quad, from the statistics chan_final_kernel<FinalStats> left in mean / rstd
__global__ void __launch_bounds__(TT)
bn_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long long M, int C, int ldx, int ldy, const float* __restrict__ mean,
                const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                unsigned short* __restrict__ y_bf16, const float* __restrict__ res, int ldr) {
    long long r;
    int c;
    if (!row_quad(M, C, r, c)) return;
    float alpha[4], bb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        alpha[k] = rstd[c + k] * gamma[c + k];
        bb[k] = beta[c + k] - mean[c + k] * alpha[k];
    }
    bn_apply_row(r, c, x, ldx, res, ldr, y, ldy, y_bf16, C, alpha, bb, relu);
}

// bn_bwd_row on a flat launch, one thread per row quad, from the sums chan_final_kernel<FinalParamGrad> left in sums[2][C]
__global__ void __launch_bounds__(TT)
bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ dx, long long M, int C,
                    int lddy, int ldx, int ldy, int lddx, const float* __restrict__ mean, const float* __restrict__ rstd,
                    const float* __restrict__ gamma, const double* __restrict__ sums, unsigned short* __restrict__ dx_bf16) {
    long long r;
    int c;
    if (!row_quad(M, C, r, c)) return;
    const double invM = 1.0 / (double)M;
    float mu[4], rs[4], gs[4], m1[4], m2[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mu[k] = mean[c + k]; rs[k] = rstd[c + k]; gs[k] = gamma[c + k] * rs[k];
        m1[k] = (float)(sums[c + k] * invM); m2[k] = (float)(sums[C + c + k] * invM);
    }
    bn_bwd_row(r, c, dy, lddy, x, ldx, y, ldy, dx, lddx, dx_bf16, C, mu, rs, gs, m1, m2, o);
}

// ---- BatchNorm in eval() mode (frozen: the running statistics are read, never written) --------------------------------------------------
// invstd of a frozen channel: 1 / sqrt(running_var + eps) formed in fp64 and rounded once, by ONE thread per channel and workgroup (an fp64
// sqrt and division per row quad would make these HBM-bound passes compute-bound); a workgroup then shares its 64 channels' constants in LDS.
__device__ __forceinline__ float bn_eval_rstd(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }

// y = relu?((x - running_mean) * rstd * gamma + beta + res): bn_apply_row with alpha = fl(rstd * gamma), bb = fl(beta - fl(running_mean * alpha)),
// the arithmetic of bn_apply_kernel on the running statistics.  64 rows x 64 channels per workgroup (16 channel quads x 16 row-lanes, 4 rows each).
__global__ void __launch_bounds__(TT)
bn_eval_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long long M, int C, int ldx, int ldy, const float* __restrict__ running_mean,
                     const float* __restrict__ running_var, float eps, const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                     const float* __restrict__ res, int ldr) {
    __shared__ float alpha_s[64], bb_s[64];
    const int c0 = blockIdx.y * 64;
    const long long m0 = (long long)blockIdx.x * 64;
    if (threadIdx.x < 64 && c0 + threadIdx.x < C) {
        const int cc = c0 + threadIdx.x;
        const float a = bn_eval_rstd(running_var[cc], eps) * gamma[cc];
        alpha_s[threadIdx.x] = a;
        bb_s[threadIdx.x] = beta[cc] - running_mean[cc] * a;
    }
    __syncthreads();
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = c0 + cq * 4;
    if (c >= C) return;
    float alpha[4], bb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { alpha[k] = alpha_s[cq * 4 + k]; bb[k] = bb_s[cq * 4 + k]; }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const long long r = m0 + rl + 16 * rr;
        if (r < M) bn_apply_row(r, c, x, ldx, res, ldr, y, ldy, nullptr, C, alpha, bb, relu);
    }
}

// The backward of the frozen form: g' = dy * (y > 0) (y != NULL), dx = g' * gs with gs = fl(gamma * rstd) -- no reduction behind it -- and, SUMS,
// the chunk sums of dbeta = S g' and dgamma = S g' * xh in chan_partial_kernel<1>'s grid, block layout, operands (bn_bwd_operands) and summation
// order, which chan_final_kernel<FinalParamGrad> then adds up: the pass that accumulates them writes dx (dx == NULL: sums only).  !SUMS: x is not
// read, nothing but dx is written, and the rows are split over blockIdx.x (no chunk grid: blockIdx.y could not count the row blocks of a large map).
template <bool SUMS>
__global__ void __launch_bounds__(TT)
bn_eval_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ dx, long long M, int C,
                   int lddy, int ldx, int ldy, int lddx, const float* __restrict__ running_mean, const float* __restrict__ running_var, float eps,
                   const float* __restrict__ gamma, int rows_per_chunk, double* __restrict__ partial) {
    __shared__ double red[SUMS ? 2 : 1][SUMS ? 16 : 1][64];
    __shared__ float mu_s[64], rs_s[64], gs_s[64];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int cblk = SUMS ? blockIdx.x : blockIdx.y, chunk = SUMS ? blockIdx.y : blockIdx.x;
    const int c = cblk * 64 + cq * 4;
    const long long r0 = (long long)chunk * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    if (threadIdx.x < 64 && cblk * 64 + threadIdx.x < C) {
        const int cc = cblk * 64 + threadIdx.x;
        const float rs = bn_eval_rstd(running_var[cc], eps);
        mu_s[threadIdx.x] = running_mean[cc];
        rs_s[threadIdx.x] = rs;
        gs_s[threadIdx.x] = dx ? gamma[cc] * rs : 0.f;
    }
    __syncthreads();
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    if (c < C) {
        float mu[4], rs[4], gs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { mu[k] = mu_s[cq * 4 + k]; rs[k] = rs_s[cq * 4 + k]; gs[k] = gs_s[cq * 4 + k]; }
        for (long long r = r0 + rl; r < r1; r += 16) {
            float g[4];
            load4(dy + r * lddy + c, g);
            if (SUMS) {
                float xh[4];
                bn_bwd_operands(g, xh, r, c, x, ldx, y, ldy, mu, rs);
#pragma unroll
                for (int k = 0; k < 4; ++k) { s0[k] += (double)g[k]; s1[k] += (double)g[k] * (double)xh[k]; }
            } else if (y) {
                float yv[4];
                load4(y + r * ldy + c, yv);
                relu_mask4(g, yv);
            }
            if (dx) {
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = g[k] * gs[k];
                store4(dx + r * lddx + c, o);
            }
        }
    }
    if constexpr (SUMS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[0][rl][cq * 4 + k] = s0[k]; red[1][rl][cq * 4 + k] = s1[k]; }
        __syncthreads();
        if (threadIdx.x < 128) {                   // chan_partial_kernel's: 64 channels x 2 sums; row-lanes added in order 0..15
            const int q = threadIdx.x >> 6, l = threadIdx.x & 63, cc = cblk * 64 + l;
            if (cc < C) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < 16; ++j) t += red[q][j][l];
                partial[((size_t)chunk * 2 + q) * C + cc] = t;
            }
        }
    }
}

// bn_bwd_row on 64 pixels x 64 channels per workgroup, which ALSO writes the transpose of dx as plain bf16 rows [C][Mp] (zero for
// m >= M): dx of the BatchNorm behind a conv is that conv's dY, and its weight-gradient GEMM reads dY^T in exactly this format
// (vidc_im2col_transposed(..., KH = KW = 1, split = 2) -- one launch and one pass over dY per conv that this kernel makes unnecessary).
// LDS tile [pixel][channel], pitch 65 floats, both phases as in im2col_t64_kernel; every value is rounded once, from the fp32 result.
// FOLD: `sums` holds the CHUNK sums of chan_partial_kernel<1> (n_chunks of them) and the workgroup adds them up itself for its 64 channels
// (column_sums: chan_final's order); the workgroups of the first pixel block write dgamma / dbeta.  dx_bf16_t may then be NULL (no
// transposed copy wanted): the kernel is the folded form of bn_bwd_apply_kernel as well.
template <bool FOLD>
__global__ void __launch_bounds__(256)
bn_bwd_apply_t64_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ dx, int M, int C,
                        int lddy, int ldx, int ldy, int lddx, const float* __restrict__ mean, const float* __restrict__ rstd,
                        const float* __restrict__ gamma, const double* __restrict__ sums, unsigned short* __restrict__ dx_bf16,
                        unsigned short* __restrict__ dx_bf16_t, int Mp, int n_chunks, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    // (FOLD: the reduction scratch [2][32][64] doubles and the transpose tile [64][65] floats share the same LDS, one after the other)
    __shared__ __attribute__((aligned(16))) unsigned char raw_s[FOLD ? 2 * 32 * 64 * 8 : 64 * 65 * 4];
    __shared__ double sum_s[2][64];
    float (*tile)[65] = reinterpret_cast<float (*)[65]>(raw_s);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int c = c0 + tx * 4;
    const double invM = 1.0 / (double)M;
    if (FOLD) {
        double (*red)[32][64] = reinterpret_cast<double (*)[32][64]>(raw_s);
        column_sums(sums, n_chunks, C, c0, red);
        if (threadIdx.x < 128) {
            const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
            const double t = c0 + l < C ? red[q][0][l] : 0.0;
            sum_s[q][l] = t;
            if (blockIdx.x == 0 && c0 + l < C) (q ? dgamma : dbeta)[c0 + l] = (float)t;      // FinalParamGrad: dbeta = sum dy', dgamma = sum dy' * xhat
        }
        __syncthreads();
    }
    float mu[4], rs[4], gs[4], m1[4], m2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ck = c + k < C ? c + k : C - 1;
        mu[k] = mean[ck]; rs[k] = rstd[ck]; gs[k] = gamma[ck] * rs[k];
        const double t0 = FOLD ? sum_s[0][ck - c0] : sums[ck], t1 = FOLD ? sum_s[1][ck - c0] : sums[C + ck];
        m1[k] = (float)(t0 * invM); m2[k] = (float)(t1 * invM);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + ty + 16 * r;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (m < M && c < C) bn_bwd_row(m, c, dy, lddy, x, ldx, y, ldy, dx, lddx, dx_bf16, C, mu, rs, gs, m1, m2, o);
        float* t = &tile[ty + 16 * r][tx * 4];
        t[0] = o[0]; t[1] = o[1]; t[2] = o[2]; t[3] = o[3];
    }
    if (!dx_bf16_t) return;               // (uniform over the launch)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cl = ty + 16 * r, cc = c0 + cl, m = m0 + tx * 4;
        if (cc < C && m < Mp) {
            const float v[4] = {tile[tx * 4][cl], tile[tx * 4 + 1][cl], tile[tx * 4 + 2][cl], tile[tx * 4 + 3][cl]};
            store4_bf16(dx_bf16_t + (size_t)cc * Mp + m, v);
        }
    }
}

// ---- elementwise ---------------------------------------------------------------------------------------------------------------
// y = relu?(a + b)  (Bottleneck: out = relu(bn3(conv3) + identity); decoder: z1 + z2 + z3 + z4 without ReLU)
__global__ void __launch_bounds__(TT)
add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long long M, int C, int lda, int ldb, int ldy, int relu,
           unsigned short* __restrict__ y_bf16) {
    long long r;
    int c;
    if (!row_quad(M, C, r, c)) return;
    float u[4], v[4], o[4];
    load4(a + r * lda + c, u);
    load4(b + r * ldb + c, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = u[k] + v[k];
    if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
    }
    store4(y + r * ldy + c, o);
    if (y_bf16) store4_bf16(y_bf16 + r * C + c, o);      // the bf16 operand copy (dense rows) the convs of the next block read in a VIDC_PREC_BF16 step
}

// dx (=|+=) dy * (y > 0)   (y NULL: plain copy / accumulate)
__global__ void __launch_bounds__(TT)
relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long long M, int C, int lddy, int ldy, int lddx, int accumulate) {
    long long r;
    int c;
    if (!row_quad(M, C, r, c)) return;
    float g[4];
    load4(dy + r * lddy + c, g);
    if (y) {
        float v[4];
        load4(y + r * ldy + c, v);
        relu_mask4(g, v);
    }
    float* d = dx + r * lddx + c;
    if (accumulate) {
        float o[4];
        load4(d, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += o[k];
    }
    store4(d, g);
}

// ---- gather kernels over the pixels of an NHWC tensor: one thread per V consecutive channels of a pixel ----------------------------
// V = 4: a row quad through 16-byte accesses and 32-bit offsets (C and the strides multiples of 4, 16-byte aligned tensors below 2^31
// elements: the pyramids' 64-channel maps; the host entry points check).  V = 1: any C, stride and size, 64-bit offsets.  Per channel both
// instantiations of a kernel scan and add in the same order: identical bits.
template <int V>
struct Lanes {
    using Index = typename std::conditional<V == 1, long long, unsigned>::type;
    static __device__ __forceinline__ void load(const float* __restrict__ p, float* v) {
        if constexpr (V == 4) load4(p, v); else v[0] = *p;
    }
    static __device__ __forceinline__ void store(float* __restrict__ p, const float* v) {
        if constexpr (V == 4) store4(p, v); else *p = v[0];
    }
    // thread -> pixel (b, y, x) of a B x H x W x C tensor and first channel c; false for the threads past the end
    static __device__ __forceinline__ bool pixel(int B, int H, int W, int C, int& b, int& y, int& x, int& c) {
        const int cv = C / V;
        const Index i = (Index)blockIdx.x * TT + threadIdx.x;
        if (i >= (Index)B * H * W * cv) return false;
        c = (int)(i % cv) * V;
        Index p = i / cv;
        x = (int)(p % W); p /= W;
        y = (int)(p % H);
        b = (int)(p / H);
        return true;
    }
    // element offset of channel c of pixel (b, y, x), rows of ld channels
    static __device__ __forceinline__ Index at(int b, int y, int x, int H, int W, int ld, int c) { return (((Index)b * H + y) * W + x) * (Index)ld + c; }
};

// ---- max-pool 3x3 / stride 2 / pad 1 backward (gather, deterministic) -------------------------------------------------------------
// An input pixel receives dy of every window whose FIRST maximum (scan order kh, kw like torch's CPU kernel) it is.
template <int V>
__global__ void __launch_bounds__(TT)
maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int B, int H, int W, int C, int ldx, int lddy, int lddx) {
    using L = Lanes<V>;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    int b, h, w, c;
    if (!L::pixel(B, H, W, C, b, h, w, c)) return;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int oy = h / 2; oy <= (h + 1) / 2; ++oy) {       // the windows with 2*oy-1 <= h <= 2*oy+1: one for even h, two for odd h
        if (oy >= Ho) continue;
        for (int ox = w / 2; ox <= (w + 1) / 2; ++ox) {
            if (ox >= Wo) continue;
            float best[V];
            int first[V];                                 // kh * 3 + kw of the first maximum
#pragma unroll
            for (int k = 0; k < V; ++k) { best[k] = -INFINITY; first[k] = -1; }
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = 2 * oy - 1 + kh;
                if (ih < 0 || ih >= H) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = 2 * ox - 1 + kw;
                    if (iw < 0 || iw >= W) continue;
                    float v[V];
                    L::load(x + L::at(b, ih, iw, H, W, ldx, c), v);
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        if (v[k] > best[k] || first[k] < 0) { best[k] = v[k]; first[k] = kh * 3 + kw; }
                }
            }
            const int mine = (h - (2 * oy - 1)) * 3 + (w - (2 * ox - 1));
            float g[V];
            L::load(dy + L::at(b, oy, ox, Ho, Wo, lddy, c), g);
#pragma unroll
            for (int k = 0; k < V; ++k) if (first[k] == mine) acc[k] += g[k];
        }
    }
    L::store(dx + L::at(b, h, w, H, W, lddx, c), acc);
}

// ---- bilinear upsampling (align_corners = True) backward, gather form ------------------------------------------------------------
// Forward (pointwise.hip / F.interpolate): src = dst * (in - 1) / (out - 1) in fp32, i0 = floor(src), i1 = min(i0 + 1, in - 1),
// lambda = src - i0.  The input pixel (i, j) collects every output pixel that interpolated from it.
__device__ inline void up_src(int d, int in, int out, int& i0, int& i1, float& lam) {
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    const float s = scale * (float)d;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    lam = s - (float)i0;
}
// (the interpolation weights of a pixel are computed once for its V channels)
template <int V>
__global__ void __launch_bounds__(TT)
upsample_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int h, int w, int C, int lddy, int lddx, int H, int W) {
    using L = Lanes<V>;
    int b, ii, jj, c;
    if (!L::pixel(B, h, w, C, b, ii, jj, c)) return;
    // candidate output rows: src in (ii - 1, ii + 1)  ->  dst in ((ii-1)/scale, (ii+1)/scale); scanned with a margin of one
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    int Y0 = 0, Y1 = H - 1, X0 = 0, X1 = W - 1;
    if (sy > 0.f) { Y0 = max(0, (int)floorf((float)(ii - 1) / sy) - 1); Y1 = min(H - 1, (int)ceilf((float)(ii + 1) / sy) + 1); }
    if (sx > 0.f) { X0 = max(0, (int)floorf((float)(jj - 1) / sx) - 1); X1 = min(W - 1, (int)ceilf((float)(jj + 1) / sx) + 1); }
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int Y = Y0; Y <= Y1; ++Y) {
        int a0, a1; float ly;
        up_src(Y, h, H, a0, a1, ly);
        const float wy = (a0 == ii ? 1.f - ly : 0.f) + (a1 == ii ? ly : 0.f);
        if (wy == 0.f) continue;
        for (int X = X0; X <= X1; ++X) {
            int b0, b1; float lx;
            up_src(X, w, W, b0, b1, lx);
            const float wx = (b0 == jj ? 1.f - lx : 0.f) + (b1 == jj ? lx : 0.f);
            if (wx == 0.f) continue;
            float g[V];
            L::load(dy + L::at(b, Y, X, H, W, lddy, c), g);
            const float ww = wy * wx;
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += ww * g[k];
        }
    }
    L::store(dx + L::at(b, ii, jj, h, w, lddx, c), acc);
}

// ---- nn.AvgPool2d(k, stride, padding), count_include_pad=True, backward (surface_normal_dorn.py:10), gather form -----------------------
// Forward (pointwise.hip): y[b,oy,ox,c] = (sum of the window's pixels inside the image) / (kh*kw).  One thread owns dx[b,y,x,c..c+3] and adds
// dy[b,oy,ox,c..c+3] / (kh*kw) over the windows that contain (y, x), oy then ox ascending: overlapping windows (stride < kernel) add up,
// a pixel no window covers (rows / columns past the last whole window) gets 0, and the order is fixed, so the result is bit-reproducible.
// 16-byte loads and stores along C; the kernel moves |dx| + |dy| bytes and does nothing else.
__global__ void __launch_bounds__(TT)
avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int H, int W, int C, int lddx, int kh, int kw, int sh, int sw, int ph,
                   int pw, int Ho, int Wo, int lddy) {
    const int q = C >> 2;
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    if (i >= (long long)B * H * W * q) return;
    const int c = (int)(i % q) * 4;
    long long p = i / q;
    const int xx = (int)(p % W); p /= W;
    const int yy = (int)(p % H);
    const int b = (int)(p / H);
    // window oy covers rows oy*sh - ph .. oy*sh - ph + kh - 1:  (yy + ph - kh + 1) / sh rounded up <= oy <= (yy + ph) / sh rounded down
    const int ty = yy + ph, tx = xx + pw;
    const int oy0 = ty >= kh ? (ty - kh + sh) / sh : 0, oy1 = min(Ho - 1, ty / sh);
    const int ox0 = tx >= kw ? (tx - kw + sw) / sw : 0, ox1 = min(Wo - 1, tx / sw);
    const float d = (float)(kh * kw);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const float4 g = *reinterpret_cast<const float4*>(dy + ((size_t)(b * Ho + oy) * Wo + ox) * lddy + c);
            acc.x += g.x / d; acc.y += g.y / d; acc.z += g.z / d; acc.w += g.w / d;
        }
    *reinterpret_cast<float4*>(dx + ((size_t)(b * H + yy) * W + xx) * lddx + c) = acc;
}

// ---- 1x1 head conv with Cout <= 4 output channels and any padding: backward ---------------------------------------------------------
// (depth_completion.py:141-147: Conv2d(192, 1, 1, padding=1); surface_normal.py:143: Conv2d(64, 3, 1))
// g_low: [B*Cout][h+2p][w+2p] planes (the layout of vidc_head_conv1x1_upsample's lowres); x: NHWC [B][h][w][C]; wgt: [Cout][C].
constexpr int kRowsPerChunk = 256;        // rows per workgroup of the per-channel reductions: M = 10^4..10^5 rows -> hundreds of workgroups per 64 channels
constexpr int kFinalLanes = 32;
constexpr int kMaxCout = 4;

// dx[b,y,x,c] = sum_o g_low[b,o,y+p,x+p] * w[o][c], o ascending
__global__ void __launch_bounds__(TT)
head_dgrad_kernel(const float* __restrict__ g_low, const float* __restrict__ wgt, float* __restrict__ dx, int B, int h, int w, int C, int Cout, int pad,
                  int lddx) {
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    const long long total = (long long)B * h * w * C;
    if (i >= total) return;
    const int c = (int)(i % C);
    long long p = i / C;
    const int xx = (int)(p % w); p /= w;
    const int yy = (int)(p % h);
    const int b = (int)(p / h);
    const int wp = w + 2 * pad;
    const long long plane = (long long)(h + 2 * pad) * wp;
    const float* g = g_low + (long long)b * Cout * plane + (long long)(yy + pad) * wp + xx + pad;
    float acc = g[0] * wgt[c];
    for (int o = 1; o < Cout; ++o) acc = fmaf(g[o * plane], wgt[o * C + c], acc);
    dx[(((long long)b * h + yy) * w + xx) * lddx + c] = acc;
}

// partial[chunk][o][c] = sum over the chunk's rows of g_low_interior[o] * x[.., c]; one block per channel chunk would re-read g: here one
// thread per (chunk, c), fp64
__global__ void __launch_bounds__(TT)
head_wgrad_partial_kernel(const float* __restrict__ g_low, const float* __restrict__ x, int B, int h, int w, int C, int Cout, int pad, int ldx,
                          double* __restrict__ partial) {
    const int c = blockIdx.x * TT + threadIdx.x;
    if (c >= C) return;
    const long long M = (long long)B * h * w;
    const long long r0 = (long long)blockIdx.y * kRowsPerChunk, r1 = min(M, r0 + kRowsPerChunk);
    const int wp = w + 2 * pad;
    const long long plane = (long long)(h + 2 * pad) * wp;
    double s[kMaxCout] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r0; r < r1; ++r) {
        const int xx = (int)(r % w);
        const long long q = r / w;
        const int yy = (int)(q % h), b = (int)(q / h);
        const float* g = g_low + (long long)b * Cout * plane + (long long)(yy + pad) * wp + xx + pad;
        const double xv = (double)x[r * ldx + c];
#pragma unroll
        for (int o = 0; o < kMaxCout; ++o)
            if (o < Cout) s[o] += (double)g[o * plane] * xv;
    }
#pragma unroll
    for (int o = 0; o < kMaxCout; ++o)
        if (o < Cout) partial[((size_t)blockIdx.y * Cout + o) * C + c] = s[o];
}

// n_out outputs (the head's Cout * C, the stem's Cout * Cin * 9); kFinalLanes lanes per output: lane j sums chunks j, j + kFinalLanes, ... and
// the lanes' sums are added in the order j = 0, 1, ... -- a fixed order, so the result is reproducible; one lane per output walked up to 600
// chunks serially (120 us on the critical path of every pyramid's stem).
__global__ void __launch_bounds__(TT) head_wgrad_final_kernel(const double* __restrict__ partial, int n_chunks, int n_out, float* __restrict__ dw) {
    __shared__ double red[kFinalLanes][TT / kFinalLanes];
    const int l = threadIdx.x % (TT / kFinalLanes), j = threadIdx.x / (TT / kFinalLanes);
    const int c = blockIdx.x * (TT / kFinalLanes) + l;
    double s = 0.0;
    if (c < n_out)
        for (int k = j; k < n_chunks; k += kFinalLanes) s += partial[(size_t)k * n_out + c];
    red[j][l] = s;
    __syncthreads();
    if (j == 0 && c < n_out) {
        double t = red[0][l];
#pragma unroll
        for (int q = 1; q < kFinalLanes; ++q) t += red[q][l];
        dw[c] = (float)t;
    }
}

// ---- fixed-order fp64 sums of float planes: the loss (one plane) and the head's bias gradient ---------------------------------------
// v: [B][n_planes][plane].  partial[o][blockIdx.x] = this workgroup's share of the sum over b of plane o = blockIdx.y (for the head that is
// the WHOLE padded plane: a padded 1x1 conv's border outputs are the bias); kSumPer values per thread.
constexpr int kSumPer = 16;
inline int sum_blocks(long long n) { return (int)((n + (long long)TT * kSumPer - 1) / ((long long)TT * kSumPer)); }
__global__ void __launch_bounds__(TT) sum_partial_kernel(const float* __restrict__ v, int B, int n_planes, long long plane, double* __restrict__ partial) {
    __shared__ double red[1][TT];
    const int o = blockIdx.y;
    const long long n = (long long)B * plane, base = (long long)blockIdx.x * TT * kSumPer;
    double s = 0.0;
    for (int k = 0; k < kSumPer; ++k) {
        const long long i = base + (long long)k * TT + threadIdx.x;
        if (i < n) {
            const long long b = i / plane;
            s += (double)v[(b * n_planes + o) * plane + (i - b * plane)];
        }
    }
    red[0][threadIdx.x] = s;
    block_tree<1>(red);
    if (threadIdx.x == 0) partial[(size_t)o * gridDim.x + blockIdx.x] = red[0][0];
}
// one workgroup per plane: its nb partials in a fixed order
__global__ void __launch_bounds__(TT) sum_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out_d, float* __restrict__ out_f) {
    __shared__ double red[1][TT];
    const double* p = partial + (size_t)blockIdx.x * nb;
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += TT) s += p[i];
    red[0][threadIdx.x] = s;
    block_tree<1>(red);
    if (threadIdx.x == 0) { if (out_d) out_d[blockIdx.x] = red[0][0]; if (out_f) out_f[blockIdx.x] = (float)red[0][0]; }
}

// ---- masked L1 loss (network_run.py:163-173): terms |pred - gt| / (H*W) on gt > 0, and d loss / d pred ----------------------------
__global__ void __launch_bounds__(TT)
l1_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long long n, float inv_hw, float* __restrict__ terms, float* __restrict__ dpred) {
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const float g = gt[i], d = pred[i] - g;
    const bool on = g > 0.f;
    terms[i] = on ? fabsf(d) * inv_hw : 0.f;
    dpred[i] = on ? (d > 0.f ? inv_hw : (d < 0.f ? -inv_hw : 0.f)) : 0.f;
}

// ---- Adam (torch.optim.Adam defaults: no weight decay, no amsgrad) on a flat parameter buffer -------------------------------------
// One element: adam_one (optim.h; csrc/optim.hip runs the same update with weight decay, clipping and parameter groups).
// 28 bytes per parameter (p, g, m, v in; p, m, v out): one thread per four consecutive parameters (16-byte accesses), the n % 4 tail scalar
__global__ void __launch_bounds__(TT)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n, float lr, float b1, float b2,
            float eps, float bc1, float bc2_sqrt) {
    const long long i = ((long long)blockIdx.x * TT + threadIdx.x) * 4;
    if (i >= n) return;
    const float c1 = 1.f - b1, c2 = 1.f - b2, step_size = lr / bc1;
    if (i + 4 <= n) {
        float4 pv = *reinterpret_cast<float4*>(p + i), mv = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
        const float4 gv = *reinterpret_cast<const float4*>(g + i);
        adam_one(pv.x, gv.x, mv.x, vv.x, b1, b2, c1, c2, eps, step_size, bc2_sqrt);
        adam_one(pv.y, gv.y, mv.y, vv.y, b1, b2, c1, c2, eps, step_size, bc2_sqrt);
        adam_one(pv.z, gv.z, mv.z, vv.z, b1, b2, c1, c2, eps, step_size, bc2_sqrt);
        adam_one(pv.w, gv.w, mv.w, vv.w, b1, b2, c1, c2, eps, step_size, bc2_sqrt);
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
        *reinterpret_cast<float4*>(p + i) = pv;
    } else {
        for (long long k = i; k < n; ++k) adam_one(p[k], g[k], m[k], v[k], b1, b2, c1, c2, eps, step_size, bc2_sqrt);
    }
}

// ---- dgrad helpers -------------------------------------------------------------------------------------------------------------
// Weights of the dgrad convolution, packed for conv_mfma.hip: the conv computing dX from dY has Cout' = Cin, Cin' = Cout and the
// kernel flipped: wp[ci][co/32][KH-1-kh][KW-1-kw][co%32] = w[co][ci][kh][kw]  (wp is [Cout'][Cin'/32][KH][KW][32]).
__global__ void __launch_bounds__(TT)
pack_weight_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int KH, int KW) {
    const long long total = (long long)Cout * Cin * KH * KW;
    const long long idx = (long long)blockIdx.x * TT + threadIdx.x;
    if (idx >= total) return;
    const int Kp = Cout * KH * KW;                     // K of the dgrad conv
    const int ci = (int)(idx / Kp), k = (int)(idx - (long long)ci * Kp);
    const int lane = k & 31, u = k >> 5, taps = KH * KW;
    const int cu = u / taps, tap = u - cu * taps, kh = tap / KW, kw = tap - kh * KW, co = cu * 32 + lane;
    wp[idx] = w[(((long long)co * Cin + ci) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)];
}
// Every conv weight of a network re-packed in ONE launch (the parameters move every optimizer step): block -> item by binary search over
// items[].block_begin (uniform per block: scalar loads).  Both maps are staged through LDS so that the parameter is read and the packed
// copy written in contiguous runs:
//  forward (kind & 1 == 0): a U-channel K unit of a row is the same U*taps contiguous elements in the parameter ([U][taps]) and in the
//      packed row ([taps][U]) -- a local transpose; a block does kPackUnits of them (for a 1x1 conv it is a copy);
//  dgrad (kind & 1): a block takes U output channels x kPackCi input channels: U contiguous runs of kPackCi*taps parameter elements in,
//      kPackCi*taps runs of U packed elements out (kernel flipped).
// U = 32 channels per 128-byte unit for fp32 / split-bf16 ([32 x hi | 32 x lo]), 64 for plain bf16.
// (a 1x1 conv has 1/9 of the elements per unit / per input channel: its blocks take 64 of them instead of 8 -- with 8 a block moved 256-512
//  elements and the launch, ~600 000 blocks for the 310 M parameters, was bound by block start-up and the item search, not by bandwidth)
constexpr int kPackUnits = 8, kPackCi = 8;
__host__ __device__ inline int pack_units(int taps) { return taps == 1 ? 64 : kPackUnits; }
__host__ __device__ inline int pack_ci(int taps) { return taps == 1 ? 64 : kPackCi; }
__host__ __device__ inline long long pack_item_blocks(int Cout, int Cin, int KH, int KW, int kind) {
    const int U = (kind & 4) ? 64 : 32, pu = pack_units(KH * KW), pc = pack_ci(KH * KW);
    if (!(kind & 1)) return ((long long)Cout * (Cin / U) + pu - 1) / pu;
    return (long long)(Cout / U) * ((Cin + pc - 1) / pc);
}
__device__ inline void pack_store(const vidc_pack_item& it, long long off, float v) {
    if (it.kind & 4) {
        reinterpret_cast<unsigned short*>(it.packed)[off] = vidc::bf16_rne(v);
    } else if (it.kind & 2) {
        unsigned short h, l;
        vidc::split_bf16(v, h, l);
        unsigned short* base = reinterpret_cast<unsigned short*>(it.packed) + (off >> 5) * 64 + (off & 31);
        base[0] = h;
        base[32] = l;
    } else {
        it.packed[off] = v;
    }
}
// Round 4, plain-bf16 kinds (the training mode configs[4] names; 1.41 ms for the 310 M parameters before): a thread produces eight
// consecutive bf16 values and stores them at once (2-byte stores before), and a 1x1 forward copy -- the same order as the parameter --
// skips the LDS round trip: 0.79 ms (4.7 TB/s).  Same values.  (A block -> item index instead of the search over block_begin was
// measured too: 0.79 against 0.76 ms, nothing -- the table is cache-resident and the search overlaps other blocks' traffic.)
constexpr int kPackTile = 64 * (kPackCi * 9 + 1);         // 64 channels x (8 x 9 + 1) floats = 18.25 KB; also holds 8 units x 64 x 9, 64 units x 64 x 1
static_assert(64 * 64 <= kPackTile && 64 * (64 + 1) <= kPackTile, "1x1 blocks must fit the tile");
// block lb of item `it` (both uniform per workgroup); tile: kPackTile floats of LDS.  One body for the batched launch and for pack_one_kernel.
__device__ inline void pack_block(const vidc_pack_item& it, int lb, float* tile) {
    const int taps = it.KH * it.KW, U = (it.kind & 4) ? 64 : 32, seg = U * taps;
    const bool plain = (it.kind & 4) != 0;                  // plain bf16: U == 64
    if (!(it.kind & 1)) {
        const int pu = pack_units(taps);
        const long long units = (long long)it.Cout * (it.Cin / U), u0 = (long long)lb * pu;
        const int cnt = (int)min((long long)pu, units - u0) * seg;
        const float* src = it.w + u0 * seg;
        const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;       // (a parameter sits anywhere in the flat buffer)
        if (plain && taps == 1) {                           // cnt % 64 == 0
            unsigned short* dst = reinterpret_cast<unsigned short*>(it.packed) + u0 * seg;
            for (int i = threadIdx.x * 8; i < cnt; i += TT * 8) {
                float v[8];
                if (aligned) {
                    const float4 a = *reinterpret_cast<const float4*>(src + i), b = *reinterpret_cast<const float4*>(src + i + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = src[i + k];
                }
                store8_bf16(dst + i, v);
            }
            return;
        }
        if (aligned) {                                      // cnt % 4 == 0 (seg is a multiple of 32)
            for (int i = threadIdx.x * 4; i < cnt; i += TT * 4) *reinterpret_cast<float4*>(tile + i) = *reinterpret_cast<const float4*>(src + i);
        } else {
            for (int i = threadIdx.x; i < cnt; i += TT) tile[i] = src[i];
        }
        __syncthreads();
        if (plain) {                                        // eight lanes of one tap per thread
            unsigned short* dst = reinterpret_cast<unsigned short*>(it.packed) + u0 * seg;
            for (int i = threadIdx.x * 8; i < cnt; i += TT * 8) {
                const int u = i / seg, r = i - u * seg, tap = r >> 6, lane = r & 63;
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = tile[u * seg + (lane + k) * taps + tap];
                store8_bf16(dst + i, v);
            }
        } else {
            for (int i = threadIdx.x; i < cnt; i += TT) {
                const int u = i / seg, r = i - u * seg, tap = r / U, lane = r - tap * U;
                pack_store(it, u0 * seg + i, tile[u * seg + lane * taps + tap]);
            }
        }
    } else {
        const int pc = pack_ci(taps);
        const int ci_tiles = (it.Cin + pc - 1) / pc;
        const int cu = lb / ci_tiles, ci0 = (lb - cu * ci_tiles) * pc, nci = min(pc, it.Cin - ci0);
        const int run = nci * taps, pitch = pc * taps + 1;
        if (run == 64) {                                    // (the usual 1x1 block: no division)
            for (int i = threadIdx.x; i < U * 64; i += TT) {
                const int col = i >> 6, r = i & 63;
                tile[col * pitch + r] = it.w[((long long)(cu * U + col) * it.Cin + ci0) * taps + r];
            }
        } else {
            for (int i = threadIdx.x; i < U * run; i += TT) {
                const int col = i / run, r = i - col * run;
                tile[col * pitch + r] = it.w[((long long)(cu * U + col) * it.Cin + ci0) * taps + r];
            }
        }
        __syncthreads();
        const long long Kp = (long long)it.Cout * taps;
        if (plain) {                                        // eight output channels of one (input channel, tap) per thread
            unsigned short* dst = reinterpret_cast<unsigned short*>(it.packed);
            for (int i = threadIdx.x * 8; i < run * U; i += TT * 8) {
                const int cl = i / seg, r = i - cl * seg, tap = r >> 6, lane = r & 63;
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = tile[(lane + k) * pitch + cl * taps + (taps - 1 - tap)];
                store8_bf16(dst + (long long)(ci0 + cl) * Kp + (long long)(cu * taps + tap) * U + lane, v);
            }
        } else {
            for (int i = threadIdx.x; i < run * U; i += TT) {
                const int cl = i / seg, r = i - cl * seg, tap = r / U, lane = r - tap * U;
                pack_store(it, (long long)(ci0 + cl) * Kp + (long long)(cu * taps + tap) * U + lane, tile[lane * pitch + cl * taps + (taps - 1 - tap)]);
            }
        }
    }
}
__global__ void __launch_bounds__(TT) pack_batched_kernel(const vidc_pack_item* __restrict__ items, int n) {
    __shared__ float tile[kPackTile];
    const long long blk = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].block_begin <= blk) lo = mid; else hi = mid - 1;
    }
    const vidc_pack_item it = items[lo];
    pack_block(it, (int)(blk - it.block_begin), tile);
}
// One item, its descriptor a kernel argument: what an eager caller packs per call (no descriptor table in device memory, no upload).
__global__ void __launch_bounds__(TT) pack_one_kernel(const vidc_pack_item it) {
    __shared__ float tile[kPackTile];
    pack_block(it, (int)blockIdx.x, tile);
}

// fp32 NHWC rows [rows][ldx] (C channels used) -> dense bf16 rows [rows][C] (round to nearest even); one thread per 8 channels
__global__ void __launch_bounds__(TT) cast_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, long long rows, int C, int ldx) {
    long long r;
    int c;
    if (!row_quad<8>(rows, C, r, c)) return;
    float v[8];
    load4(x + r * ldx + c, v);
    load4(x + r * ldx + c + 4, v + 4);
    store8_bf16(y + r * C + c, v);
}

// z[b, oy*s, ox*s, :] = dy[b, oy, ox, :], zero elsewhere (z is B x H x W x C, dense)
__global__ void __launch_bounds__(TT)
zero_stuff_kernel(const float* __restrict__ dy, float* __restrict__ z, int B, int Ho, int Wo, int C, int lddy, int s, int H, int W) {
    const int c4 = C >> 2;
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    const long long total = (long long)B * H * W * c4;
    if (i >= total) return;
    const int c = (int)(i % c4) * 4;
    long long p = i / c4;
    const int x = (int)(p % W); p /= W;
    const int y = (int)(p % H);
    const int b = (int)(p / H);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y % s == 0 && x % s == 0 && y / s < Ho && x / s < Wo)
        v = *reinterpret_cast<const float4*>(dy + (((long long)b * Ho + y / s) * Wo + x / s) * lddy + c);
    *reinterpret_cast<float4*>(z + (((long long)b * H + y) * W + x) * C + c) = v;
}

// ---- wgrad: dW[co][ci][kh][kw] = sum_m dY[m][co] * X[pixel(m) shifted by the tap][ci] on the fp32 matrix cores ---------------------
// v_mfma_f32_32x32x2_f32 with the reduction index = pixel: lane l supplies A[i = l & 31][k = l >> 5] = dY[m0 + (l >> 5)][co0 + (l & 31)]
// and B[k][j] = X[.. m0 + (l >> 5) ..][ci0 + (l & 31)]: both are 32 consecutive channels of an NHWC row, i.e. coalesced 128-byte
// loads straight from global memory, no transposition, no LDS.  One wave = one 32x32 (co, ci) tile of one tap over a range of pixels;
// a workgroup = 4 waves = 2x2 tiles (64 co x 64 ci); grid = (co tiles, ci tiles * taps, pixel chunks).  Partials of the pixel chunks
// are summed in chunk order by wgrad_final_kernel (deterministic), which also writes the OIHW layout of the parameter.
typedef float f32x16 __attribute__((ext_vector_type(16)));
// One wave = a 64 x 64 (co, ci) register tile (2 x 2 MFMA tiles: 4 loads feed 4 MFMAs); a workgroup = 4 waves = 128 co x 128 ci.
__global__ void __launch_bounds__(256)
wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int lddy,
             int KH, int KW, int stride, int pad, int dil, int rows_per_chunk, float* __restrict__ partial /* [chunk][tap][Cout][Cin] */) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int taps = KH * KW;
    const int ci_tiles = (Cin + 127) / 128;
    const int tap = blockIdx.y / ci_tiles, cit = blockIdx.y - tap * ci_tiles;
    const int kh = tap / KW, kw = tap - kh * KW;
    const int co0 = blockIdx.x * 128 + (wave >> 1) * 64, ci0 = cit * 128 + (wave & 1) * 64;
    const int co[2] = {co0 + li, co0 + 32 + li}, ci[2] = {ci0 + li, ci0 + 32 + li};
    const long long M = (long long)B * Ho * Wo;
    const long long m_begin = (long long)blockIdx.z * rows_per_chunk, m_end = min(M, m_begin + rows_per_chunk);
    f32x16 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][q][r] = 0.f;
    // The pixel index of a lane advances by fixed steps, so (b, oy, ox) of the chunk's first pixel is decoded ONCE (wave-uniform: scalar
    // unit) and every lane walks from there with compares -- the first version divided twice per lane and pixel in 64-bit arithmetic,
    // ~10x the instructions of the MFMAs they fed.  Offsets are 32-bit (the host checks that both tensors stay below 2^31 elements).
    const int m_lo = (int)m_begin, m_hi = (int)m_end;
    int ox0 = m_lo % Wo, oy0 = (m_lo / Wo) % Ho, b0 = m_lo / (Wo * Ho);
    for (int m0 = m_lo; m0 < m_hi; m0 += 8) {           // 4 pixel pairs x (2 x 2) MFMAs per iteration, 16 loads in flight per lane
        float a[4][2], bv[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + 2 * t + lh;
            int ox = ox0 + 2 * t + lh, oy = oy0, b = b0;
            while (ox >= Wo) { ox -= Wo; ++oy; }
            while (oy >= Ho) { oy -= Ho; ++b; }
            a[t][0] = a[t][1] = bv[t][0] = bv[t][1] = 0.f;
            if (m < m_hi) {
                const int iy = oy * stride - pad + kh * dil, ix = ox * stride - pad + kw * dil;      // (dil: the tap spacing of a dilated conv)
                const bool inside = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const int xo = ((b * H + iy) * W + ix) * ldx;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    if (co[p] < Cout) a[t][p] = dy[m * lddy + co[p]];
                    if (inside && ci[p] < Cin) bv[t][p] = x[xo + ci[p]];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][p], bv[t][q], acc[p][q], 0, 0, 0);
        ox0 += 8;
        while (ox0 >= Wo) { ox0 -= Wo; ++oy0; }
        while (oy0 >= Ho) { oy0 -= Ho; ++b0; }
    }
    // C/D layout: col j = lane & 31, row i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float* out = partial + ((size_t)blockIdx.z * taps + tap) * (size_t)Cout * Cin;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int cj = ci0 + q * 32 + li;
            if (cj >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = co0 + p * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ro < Cout) out[(size_t)ro * Cin + cj] = acc[p][q][r];
            }
        }
}
__global__ void __launch_bounds__(TT)
wgrad_final_kernel(const float* __restrict__ partial, int n_chunks, int taps, int Cout, int Cin, float* __restrict__ dw /* OIHW */) {
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;            // index into [tap][Cout][Cin]
    const long long per = (long long)taps * Cout * Cin;
    if (i >= per) return;
    double s = 0.0;
    for (int k = 0; k < n_chunks; ++k) s += (double)partial[(size_t)k * per + i];
    const int ci = (int)(i % Cin);
    const long long q = i / Cin;
    const int co = (int)(q % Cout), tap = (int)(q / Cout);
    dw[((long long)co * Cin + ci) * taps + tap] = (float)s;
}

// ---- wgrad as a GEMM on the conv kernel: transposed operands ---------------------------------------------------------------------------
// dW[co][tap][ci] = sum_m dY^T[co][m] * Xt[tap*C + ci][m] is a plain "both operands K-contiguous" GEMM with K = the pixels -- exactly
// the 1x1 case of conv_mfma.hip (activations = rows of dY^T, weights = rows of Xt), which runs at several times the rate of the
// direct kernel above (LDS-tiled, split-K, fp32 or bf16x3).  The kernels below build the operands: xt[(tap*C + c)][m] = x[b, oy*s - p + kh*dil,
// ox*s - p + kw*dil, c] (0 outside the image and for m >= M; rows are Mp = M rounded up to 32 long; dil: the tap spacing of a dilated conv,
// 1 = the plain conv), through an LDS transpose so that both the NHWC reads and the row writes are coalesced.  With KH = KW = 1, s = 1,
// p = 0 it is the transpose of dY.  split & 3: 0 writes fp32 rows, 1 the split-bf16 operand format of the bf16x3 mode (vidc_split_bf16x3's
// layout; same bytes per row), 2 plain bf16 rows; split & 4: the rows in chan_major order.
// The addressing, shared by the kernels.  Source: pixel m = (b, oy, ox) reads, for the tap (kh, kw), the NHWC row `row` of x; false where the
// tap lies outside the image (row then means nothing).  Destination: the row of xt that holds channel c of a tap, tap-major (tap * C + c) or
// chan_major (c * taps + tap: the OIHW order of a weight gradient).
__device__ __forceinline__ bool im2col_src(int m, int kh, int kw, int H, int W, int Ho, int Wo, int stride, int pad, int dil, size_t& row) {
    const int ox = m % Wo, q = m / Wo, oy = q % Ho, b = q / Ho;
    const int iy = oy * stride - pad + kh * dil, ix = ox * stride - pad + kw * dil;
    row = (size_t)(b * H + iy) * W + ix;
    return (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
}
__device__ __forceinline__ size_t im2col_row(bool chan_major, int c, int tap, int taps, int C) {
    return chan_major ? (size_t)c * taps + tap : (size_t)tap * C + c;
}

// 32 pixels x 32 channels per workgroup, element by element: any C, ldx and alignment.
__global__ void __launch_bounds__(256)
im2col_t_kernel(const float* __restrict__ x, float* __restrict__ xt, int B, int H, int W, int C, int ldx, int Ho, int Wo, int KH, int KW, int stride,
                int pad, int dil, int M, int Mp, int split) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tap = blockIdx.z;
    const int kh = tap / KW, kw = tap - kh * KW;
    const bool chan_major = split & 4;
    split &= 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + ty + 8 * r, c = c0 + tx;
        float v = 0.f;
        size_t row;
        if (m < M && c < C && im2col_src(m, kh, kw, H, W, Ho, Wo, stride, pad, dil, row)) v = x[row * ldx + c];
        tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ty + 8 * r, m = m0 + tx;
        if (c < C && m < Mp) {
            const float v = tile[tx][ty + 8 * r];
            const size_t row = im2col_row(chan_major, c, tap, KH * KW, C);
            if (split == 2) {
                reinterpret_cast<unsigned short*>(xt)[row * Mp + m] = vidc::bf16_rne(v);
            } else if (split) {  // the 32 pixels of this tile are one K unit of the GEMM: [32 x hi | 32 x lo] in the same 128 bytes
                unsigned short h, l;
                vidc::split_bf16(v, h, l);
                unsigned short* u = reinterpret_cast<unsigned short*>(xt + row * Mp + m0);
                u[tx] = h;
                u[32 + tx] = l;
            } else {
                xt[row * Mp + m] = v;
            }
        }
    }
}
// The same map on 64 pixels x 64 channels per workgroup, one row quad per thread in and four pixels of a row of xt out (C % 4 == 0, ldx % 4 == 0,
// aligned pointers; Mp % 32 == 0 makes every 4-pixel group of a row all-inside or all-outside).  LDS tile [pixel][channel] with an odd-word
// row pitch: the 4 x 16 lanes of a wave hit 64 different banks in both phases.
// T = float: the fp32 tensor, every output format.  T = unsigned short: the bf16 operand copy of x (dense rows of C bf16, what the forward conv
// of the plain-bf16 mode read) to plain bf16 rows -- half the bytes in and no rounding step; the copy holds the rounded values, so the bits are
// those of the fp32 form with split = 2.
template <typename T>
__global__ void __launch_bounds__(256)
im2col_t64_kernel(const T* __restrict__ x, T* __restrict__ xt, int B, int H, int W, int C, int ldx, int Ho, int Wo, int KH, int KW, int stride, int pad,
                  int dil, int M, int Mp, int split) {
    constexpr bool kBf16 = sizeof(T) == 2;
    __shared__ T tile[64][kBf16 ? 66 : 65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tap = blockIdx.z;
    const int kh = tap / KW, kw = tap - kh * KW;
    const bool chan_major = split & 4;
    split &= 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + ty + 16 * r, c = c0 + tx * 4;
        T v[4] = {0, 0, 0, 0};
        size_t row;
        if (m < M && c < C && im2col_src(m, kh, kw, H, W, Ho, Wo, stride, pad, dil, row)) load4(x + row * ldx + c, v);
        T* t = &tile[ty + 16 * r][tx * 4];
        t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cl = ty + 16 * r, c = c0 + cl, m = m0 + tx * 4;
        if (c < C && m < Mp) {
            const T v[4] = {tile[tx * 4][cl], tile[tx * 4 + 1][cl], tile[tx * 4 + 2][cl], tile[tx * 4 + 3][cl]};
            const size_t ri = im2col_row(chan_major, c, tap, KH * KW, C);
            if constexpr (kBf16) {
                store4_bf16(xt + ri * Mp + m, v);
            } else if (split == 2) {    // plain bf16 rows: 4 pixels = 8 bytes
                store4_bf16(reinterpret_cast<unsigned short*>(xt) + ri * Mp + m, v);
            } else if (split) {         // 4 pixels of one 32-pixel K unit: their hi halves and their lo halves, 8 bytes each
                unsigned short h[4], l[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) vidc::split_bf16(v[k], h[k], l[k]);
                unsigned short* u = reinterpret_cast<unsigned short*>(xt + ri * Mp + (m & ~31)) + (m & 31);
                store4_bf16(u, h);
                store4_bf16(u + 32, l);
            } else {
                store4(xt + ri * Mp + m, v);
            }
        }
    }
}
// Dense bf16 rows x[M][C] -> their transpose xt[C][Mp] (zeros for m >= M; Mp % 64 == 0): the right operand of the weight-gradient GEMM of a
// 1x1 / stride-1 conv in the plain-bf16 mode, from the bf16 operand copy its forward already read (half the bytes of the fp32 source, no
// rounding step: the bits are those vidc_im2col_transposed(split = 2) produces from the fp32 tensor, which rounds the same values).
// 64 x 64 tile through LDS, 16-byte reads along C, 32-byte runs along m out.  It is the KH = KW = 1 case of im2col_t64_kernel<unsigned short>
// and stays a kernel of its own for those widths: two loads and two stores of 16 bytes per thread where the im2col form, which must be able
// to stop at any multiple of four channels, issues four and four of 8 bytes.
__global__ void __launch_bounds__(256)
transpose_bf16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ xt, int M, int C, int Mp) {
    __shared__ unsigned short tile[64][66];
    const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    {
        const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;            // 8 channel-octets x 32 rows, two passes
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int ml = ty + 32 * r, m = m0 + ml, c = c0 + tx * 8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m < M && c < C) v = *reinterpret_cast<const uint4*>(x + (size_t)m * C + c);
            unsigned short* t = &tile[ml][tx * 8];
            t[0] = (unsigned short)v.x; t[1] = (unsigned short)(v.x >> 16); t[2] = (unsigned short)v.y; t[3] = (unsigned short)(v.y >> 16);
            t[4] = (unsigned short)v.z; t[5] = (unsigned short)(v.z >> 16); t[6] = (unsigned short)v.w; t[7] = (unsigned short)(v.w >> 16);
        }
    }
    __syncthreads();
    const int cl = threadIdx.x >> 2, seg = (threadIdx.x & 3) * 16, c = c0 + cl, m = m0 + seg;
    if (c < C && m < Mp) {
        unsigned w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = (unsigned)tile[seg + 2 * k][cl] | ((unsigned)tile[seg + 2 * k + 1][cl] << 16);
        uint4* dst = reinterpret_cast<uint4*>(xt + (size_t)c * Mp + m);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}
// dw_oihw[co][ci][tap] = tmp[co][tap * Cin + ci]
__global__ void __launch_bounds__(TT) wgrad_permute_kernel(const float* __restrict__ tmp, float* __restrict__ dw, int Cout, int Cin, int taps) {
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    const long long total = (long long)Cout * Cin * taps;
    if (i >= total) return;
    const int tap = (int)(i % taps);
    const long long q = i / taps;
    const int ci = (int)(q % Cin), co = (int)(q / Cin);
    dw[i] = tmp[((long long)co * taps + tap) * Cin + ci];
}

// stem conv (3x3, stride 2, pad 1, Cin = 1 or 3, NCHW input, no bias): dW[co][ci][kh][kw] = sum dY[m][co] * x[b][ci][2oy+kh-1][2ox+kw-1]
__global__ void __launch_bounds__(TT)
stem_wgrad_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, int B, int Cin, int H, int W, int Ho, int Wo, int Cout, int lddy,
                          int rows_per_chunk, double* __restrict__ partial /* [chunk][Cout*Cin*9] */) {
    // One thread per (co, ci) with the nine taps in registers: a row costs one dy load, nine x loads and nine fp64 multiply-adds.  (The
    // first version had one thread per (co, ci, kh, kw): ~20 instructions per multiply-add, 265 M of them -- 300 us at the end of every
    // pyramid's backward.)  Per output the rows are added in the same order as before; a tap outside the image adds dy * 0.
    const int t = blockIdx.x * TT + threadIdx.x;
    if (t >= Cout * Cin) return;
    const int ci = t % Cin, co = t / Cin;
    const long long M = (long long)B * Ho * Wo;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.0;
    int ox = (int)(r0 % Wo);                              // (b, oy, ox) of the row walk incrementally: no division in the loop
    const long long q0 = r0 / Wo;
    int oy = (int)(q0 % Ho), b = (int)(q0 / Ho);
    const float* gp = dy + r0 * lddy + co;
    const int n_rows = (int)(r1 - r0);
    const size_t plane_stride = (size_t)Cin * H * W;
    const float* plane = x + ((size_t)b * Cin + ci) * H * W;
    for (int r = 0; r < n_rows; ++r, gp += lddy) {
        const double g = (double)*gp;
        const int iy0 = 2 * oy - 1, ix0 = 2 * ox - 1;
        if (iy0 >= 0 && ix0 >= 0 && iy0 + 2 < H && ix0 + 2 < W) {      // wave-uniform: the whole 3x3 patch is inside (all but the border rows):
            const float* p0 = plane + iy0 * W + ix0;                    // nine loads at fixed offsets, no per-tap bounds logic (which was ~200
            const float* p1 = p0 + W;                                   // scalar instructions per row and bound the kernel)
            const float* p2 = p1 + W;
            const float v[9] = {p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]};
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += g * (double)v[k];
        } else {
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int iy = iy0 + kh;
                const bool row_ok = (unsigned)iy < (unsigned)H;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int ix = ix0 + kw;
                    const bool inside = row_ok && (unsigned)ix < (unsigned)W;
                    const float xv = plane[inside ? iy * W + ix : 0];
                    s[kh * 3 + kw] += g * (double)(inside ? xv : 0.f);
                }
            }
        }
        if (++ox == Wo) { ox = 0; if (++oy == Ho) { oy = 0; ++b; plane += plane_stride; } }
    }
    double* out = partial + (size_t)blockIdx.y * ((size_t)Cout * Cin * 9) + (size_t)t * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = s[k];
}

}  // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kStemRows = 64;             // rows per workgroup of vidc_stem_wgrad (M = 153 600 at batch 8: 2400 chunks of 192 threads -- the kernel is
                                          // a chain of dependent L2 latencies per thread, so it wants many short chains rather than few long ones)
inline int chunks_for(long long M) { return (int)((M + kRowsPerChunk - 1) / kRowsPerChunk); }
// Rows per workgroup of the per-channel reductions (chan_partial_kernel): about 512 workgroups per launch whatever the shape -- a function of
// (M, C) only, so the summation order of a given tensor never changes.  Multiple of 16 (the row-lanes of a block), 32..256.
inline int rows_for(long long M, int C) {
    const long long cb = (C + 63) / 64;
    long long r = (M * cb + 511) / 512;
    r = (r + 15) / 16 * 16;
    return (int)(r < 32 ? 32 : (r > 256 ? 256 : r));
}
inline int chunks_for(long long M, int C) { const int r = rows_for(M, C); return (int)((M + r - 1) / r); }
// The final reduction of a BatchNorm's chunk sums inside the consuming kernel's prologue (bn_apply_fold_kernel, bn_bwd_apply_t64_kernel<true>)
// instead of a chan_final launch: every 64 x 64 workgroup re-reads n_chunks x 64 x 2 doubles, so it is only offered where pixel blocks x
// chunks is small -- the ResNet-101 layer-3 / layer-4 maps and the coarse decoder levels, three quarters of a step's BatchNorms.  Same sums,
// same order, same bits (tests/test_training.py).  Round 4 (one thread per channel, 32 dependent loads each): 29.2 against 27.5 ms per
// batch-8 bf16 step.  Round 5 (column_sums: all 256 threads, 16 loads in flight per thread): 26.2-26.3 against 26.15 ms with per-pyramid
// lanes, 27.2 against 27.3 ms grouped -- level, as is finishing the sums by the last workgroup of each channel column of the partial-sum
// kernel (a ticket per column, tried and removed: 26.6-26.7 / 27.8 ms).  A captured step hides the 5 us chan_final launches; nothing is
// gained by removing them (profiles/r5_train_reduction_forms_ab.txt).  Hence OFF by default; the switch (vidc_train_bn_fold,
// VIDC_TRAIN_BN_FOLD=1) stays for measurements.
int g_bn_fold = 0;
inline bool fold_bn(long long M, int C) {
    return g_bn_fold && M < (1ll << 31) && ((M + 63) / 64) * (long long)chunks_for(M, C) <= 4096;
}
}

extern "C" int vidc_train_bn_fold(int enable) {
    const int prev = g_bn_fold;
    if (enable >= 0) g_bn_fold = enable ? 1 : 0;
    return prev;
}

extern "C" size_t vidc_train_scratch_bytes(long long M, int C) {
    return ((size_t)chunks_for(M, C) * 2 * (size_t)C + 2 * (size_t)C) * sizeof(double) + 256;
}

extern "C" int vidc_bn_train_forward_add(const float* x, float* y, long long M, int C, int ldx, int ldy, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, float eps, float momentum, int relu, float* save_mean, float* save_rstd,
                                         void* y_bf16, const float* residual, int ldr, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(x && y && gamma && beta && save_mean && save_rstd && scratch, VIDC_ERR_NULL, "vidc_bn_train_forward: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0 && (!residual || (ldr >= C && ldr % 4 == 0)),
                 VIDC_ERR_SHAPE, "vidc_bn_train_forward: bad shape");
    hipStream_t st = vidc::as_stream(stream);
    const int nch = chunks_for(M, C);
    double* partial = reinterpret_cast<double*>(scratch);
    double* sums = partial + (size_t)nch * 2 * C;
    hipLaunchKernelGGL(chan_partial_kernel<0>, dim3((C + 63) / 64, nch), dim3(TT), 0, st, x, (const float*)nullptr, (const float*)nullptr, M, C, ldx, 0, 0,
                       (const float*)nullptr, (const float*)nullptr, rows_for(M, C), partial);
    if (fold_bn(M, C)) {
        hipLaunchKernelGGL(bn_apply_fold_kernel, dim3((unsigned)((M + 63) / 64), (C + 63) / 64), dim3(256), 0, st, x, y, (int)M, C, ldx, ldy, partial, nch, eps,
                           momentum, save_mean, save_rstd, running_mean, running_var, gamma, beta, relu, reinterpret_cast<unsigned short*>(y_bf16), residual, ldr);
        VIDC_CHECK_LAUNCH("bn_train_forward (folded)");
        return VIDC_OK;
    }
    hipLaunchKernelGGL(chan_final_kernel<FinalStats>, dim3((C + 7) / 8), dim3(TT), 0, st, partial, nch, C, sums,
                       FinalStats{M, eps, momentum, save_mean, save_rstd, running_mean, running_var});
    hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks(M * (C / 4))), dim3(TT), 0, st, x, y, M, C, ldx, ldy, save_mean, save_rstd, gamma, beta, relu,
                       reinterpret_cast<unsigned short*>(y_bf16), residual, ldr);
    VIDC_CHECK_LAUNCH("bn_train_forward");
    return VIDC_OK;
}

// The same with the per-channel partial sums ALREADY written by the conv that produced x (VIDC_STATS_OUT: one pair of rows of C doubles per
// block of 32 output rows, in chan_partial_kernel's layout): only the final reduction and the apply pass run here.
extern "C" int vidc_bn_train_forward_stats(const float* x, float* y, long long M, int C, int ldx, int ldy, const float* gamma, const float* beta,
                                           float* running_mean, float* running_var, float eps, float momentum, int relu, float* save_mean,
                                           float* save_rstd, void* y_bf16, const float* residual, int ldr, const void* conv_stats, void* scratch,
                                           vidc_stream_t stream) {
    VIDC_REQUIRE(x && y && gamma && beta && save_mean && save_rstd && conv_stats && scratch, VIDC_ERR_NULL, "vidc_bn_train_forward_stats: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0 && (!residual || (ldr >= C && ldr % 4 == 0)),
                 VIDC_ERR_SHAPE, "vidc_bn_train_forward_stats: bad shape");
    hipStream_t st = vidc::as_stream(stream);
    const int nch = (int)((M + 31) / 32);
    double* sums = reinterpret_cast<double*>(scratch);      // [2][C]
    hipLaunchKernelGGL(chan_final_kernel<FinalStats>, dim3((C + 7) / 8), dim3(TT), 0, st, reinterpret_cast<const double*>(conv_stats), nch, C, sums,
                       FinalStats{M, eps, momentum, save_mean, save_rstd, running_mean, running_var});
    hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks(M * (C / 4))), dim3(TT), 0, st, x, y, M, C, ldx, ldy, save_mean, save_rstd, gamma, beta, relu,
                       reinterpret_cast<unsigned short*>(y_bf16), residual, ldr);
    VIDC_CHECK_LAUNCH("bn_train_forward_stats");
    return VIDC_OK;
}

extern "C" int vidc_bn_train_forward(const float* x, float* y, long long M, int C, int ldx, int ldy, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float eps, float momentum, int relu, float* save_mean, float* save_rstd,
                                     void* y_bf16, void* scratch, vidc_stream_t stream) {
    return vidc_bn_train_forward_add(x, y, M, C, ldx, ldy, gamma, beta, running_mean, running_var, eps, momentum, relu, save_mean, save_rstd, y_bf16, nullptr, 0,
                                     scratch, stream);
}

extern "C" int vidc_bn_train_backward_t(const float* dy, const float* x, const float* y_relu, float* dx, long long M, int C, int lddy, int ldx, int ldy,
                                        int lddx, const float* gamma, const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta,
                                        void* dx_bf16, void* dx_bf16_t, int Mp, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && x && gamma && save_mean && save_rstd && dgamma && dbeta && scratch, VIDC_ERR_NULL, "vidc_bn_train_backward: null pointer");
    VIDC_REQUIRE(dx || (dx_bf16 && dx_bf16_t), VIDC_ERR_NULL, "vidc_bn_train_backward: dx may be NULL only when both bf16 forms are written");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (!y_relu || ldy % 4 == 0), VIDC_ERR_SHAPE,
                 "vidc_bn_train_backward: bad shape");
    VIDC_REQUIRE(!dx_bf16_t || (Mp >= M && Mp % 64 == 0 && M < (1ll << 31) && (reinterpret_cast<uintptr_t>(dx_bf16_t) & 7) == 0), VIDC_ERR_SHAPE,
                 "vidc_bn_train_backward_t: the transposed copy has rows of Mp = M rounded up to a multiple of 64 pixels, 8-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    const int nch = chunks_for(M, C);
    double* partial = reinterpret_cast<double*>(scratch);
    double* sums = partial + (size_t)nch * 2 * C;
    hipLaunchKernelGGL(chan_partial_kernel<1>, dim3((C + 63) / 64, nch), dim3(TT), 0, st, dy, x, y_relu, M, C, lddy, ldx, ldy, save_mean, save_rstd, rows_for(M, C), partial);
    if (fold_bn(M, C)) {
        const int mp = dx_bf16_t ? Mp : (int)((M + 63) / 64 * 64);
        hipLaunchKernelGGL(bn_bwd_apply_t64_kernel<true>, dim3(mp / 64, (C + 63) / 64), dim3(256), 0, st, dy, x, y_relu, dx, (int)M, C, lddy, ldx, ldy, lddx,
                           save_mean, save_rstd, gamma, partial, reinterpret_cast<unsigned short*>(dx_bf16), reinterpret_cast<unsigned short*>(dx_bf16_t), mp, nch,
                           dgamma, dbeta);
        VIDC_CHECK_LAUNCH("bn_train_backward (folded)");
        return VIDC_OK;
    }
    hipLaunchKernelGGL(chan_final_kernel<FinalParamGrad>, dim3((C + 7) / 8), dim3(TT), 0, st, partial, nch, C, sums, FinalParamGrad{dgamma, dbeta});
    if (dx_bf16_t)
        hipLaunchKernelGGL(bn_bwd_apply_t64_kernel<false>, dim3(Mp / 64, (C + 63) / 64), dim3(256), 0, st, dy, x, y_relu, dx, (int)M, C, lddy, ldx, ldy, lddx, save_mean,
                           save_rstd, gamma, sums, reinterpret_cast<unsigned short*>(dx_bf16), reinterpret_cast<unsigned short*>(dx_bf16_t), Mp, 0,
                           (float*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks(M * (C / 4))), dim3(TT), 0, st, dy, x, y_relu, dx, M, C, lddy, ldx, ldy, lddx, save_mean, save_rstd,
                           gamma, sums, reinterpret_cast<unsigned short*>(dx_bf16));
    VIDC_CHECK_LAUNCH("bn_train_backward");
    return VIDC_OK;
}

extern "C" int vidc_bn_train_backward(const float* dy, const float* x, const float* y_relu, float* dx, long long M, int C, int lddy, int ldx, int ldy,
                                      int lddx, const float* gamma, const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta,
                                      void* dx_bf16, void* scratch, vidc_stream_t stream) {
    return vidc_bn_train_backward_t(dy, x, y_relu, dx, M, C, lddy, ldx, ldy, lddx, gamma, save_mean, save_rstd, dgamma, dbeta, dx_bf16, nullptr, 0, scratch, stream);
}

// nn.BatchNorm2d in eval() mode inside a training step (a frozen BatchNorm): one launch, nothing but y written.
extern "C" int vidc_bn_eval_forward_add(const float* x, float* y, long long M, int C, int ldx, int ldy, const float* gamma, const float* beta,
                                        const float* running_mean, const float* running_var, float eps, int relu, const float* residual, int ldr,
                                        vidc_stream_t stream) {
    VIDC_REQUIRE(x && y && gamma && beta && running_mean && running_var, VIDC_ERR_NULL, "vidc_bn_eval_forward_add: null pointer");
    VIDC_REQUIRE(M > 0 && M < (1ll << 36) && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0 &&
                 (!residual || (ldr >= C && ldr % 4 == 0)), VIDC_ERR_SHAPE, "vidc_bn_eval_forward_add: bad shape");
    hipLaunchKernelGGL(bn_eval_apply_kernel, dim3((unsigned)((M + 63) / 64), (C + 63) / 64), dim3(TT), 0, vidc::as_stream(stream), x, y, M, C, ldx, ldy,
                       running_mean, running_var, eps, gamma, beta, relu, residual, ldr);
    VIDC_CHECK_LAUNCH("bn_eval_forward");
    return VIDC_OK;
}

// Its backward: the sums (dgamma and dbeta, both or neither) and dx are each optional; without the sums it is one elementwise launch that reads
// neither x nor the scratch, with them the pass over the chunks writes dx as well and chan_final_kernel adds the chunk sums up (two launches).
extern "C" int vidc_bn_eval_backward(const float* dy, const float* x, const float* y_relu, float* dx, long long M, int C, int lddy, int ldx, int ldy,
                                     int lddx, const float* gamma, const float* running_mean, const float* running_var, float eps, float* dgamma,
                                     float* dbeta, void* scratch, vidc_stream_t stream) {
    const bool sums = dgamma || dbeta;
    VIDC_REQUIRE(dy && running_mean && running_var && (!dgamma == !dbeta) && (dx || sums) && (!dx || gamma) && (!sums || (x && scratch)), VIDC_ERR_NULL,
                 "vidc_bn_eval_backward: null pointer (dgamma and dbeta come together; x and scratch are read for them only, gamma for dx only)");
    VIDC_REQUIRE(M > 0 && M < (1ll << 36) && C > 0 && C % 4 == 0 && lddy >= C && lddy % 4 == 0 && (!x || (ldx >= C && ldx % 4 == 0)) &&
                 (!dx || (lddx >= C && lddx % 4 == 0)) && (!y_relu || (ldy >= C && ldy % 4 == 0)), VIDC_ERR_SHAPE, "vidc_bn_eval_backward: bad shape");
    hipStream_t st = vidc::as_stream(stream);
    if (!sums) {
        hipLaunchKernelGGL(bn_eval_bwd_kernel<false>, dim3((unsigned)((M + 63) / 64), (C + 63) / 64), dim3(TT), 0, st, dy, (const float*)nullptr, y_relu, dx, M, C,
                           lddy, 0, ldy, lddx, running_mean, running_var, eps, gamma, 64, (double*)nullptr);
        VIDC_CHECK_LAUNCH("bn_eval_backward (dx only)");
        return VIDC_OK;
    }
    const int nch = chunks_for(M, C);
    double* partial = reinterpret_cast<double*>(scratch);
    double* sums_d = partial + (size_t)nch * 2 * C;
    hipLaunchKernelGGL(bn_eval_bwd_kernel<true>, dim3((C + 63) / 64, nch), dim3(TT), 0, st, dy, x, y_relu, dx, M, C, lddy, ldx, ldy, lddx, running_mean,
                       running_var, eps, gamma, rows_for(M, C), partial);
    hipLaunchKernelGGL(chan_final_kernel<FinalParamGrad>, dim3((C + 7) / 8), dim3(TT), 0, st, partial, nch, C, sums_d, FinalParamGrad{dgamma, dbeta});
    VIDC_CHECK_LAUNCH("bn_eval_backward");
    return VIDC_OK;
}

extern "C" int vidc_colsum(const float* dy, long long M, int C, int ld, float* out, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && out && scratch, VIDC_ERR_NULL, "vidc_colsum: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0, VIDC_ERR_SHAPE, "vidc_colsum: bad shape (C and ld multiples of 4)");
    hipStream_t st = vidc::as_stream(stream);
    const int nch = chunks_for(M, C);
    double* partial = reinterpret_cast<double*>(scratch);
    double* sums = partial + (size_t)nch * 2 * C;
    hipLaunchKernelGGL(chan_partial_kernel<0>, dim3((C + 63) / 64, nch), dim3(TT), 0, st, dy, (const float*)nullptr, (const float*)nullptr, M, C, ld, 0, 0,
                       (const float*)nullptr, (const float*)nullptr, rows_for(M, C), partial);
    hipLaunchKernelGGL(chan_final_kernel<FinalColsum>, dim3((C + 7) / 8), dim3(TT), 0, st, partial, nch, C, sums, FinalColsum{out});
    VIDC_CHECK_LAUNCH("colsum");
    return VIDC_OK;
}

extern "C" int vidc_add_rows_bf16(const float* a, const float* b, float* y, long long M, int C, int lda, int ldb, int ldy, int relu, void* y_bf16,
                                  vidc_stream_t stream) {
    VIDC_REQUIRE(a && b && y, VIDC_ERR_NULL, "vidc_add_rows: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldy % 4 == 0, VIDC_ERR_SHAPE, "vidc_add_rows: bad shape");
    hipLaunchKernelGGL(add_kernel, dim3(blocks(M * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), a, b, y, M, C, lda, ldb, ldy, relu,
                       reinterpret_cast<unsigned short*>(y_bf16));
    VIDC_CHECK_LAUNCH("add_kernel");
    return VIDC_OK;
}

extern "C" int vidc_add_rows(const float* a, const float* b, float* y, long long M, int C, int lda, int ldb, int ldy, int relu, vidc_stream_t stream) {
    return vidc_add_rows_bf16(a, b, y, M, C, lda, ldb, ldy, relu, nullptr, stream);
}

extern "C" int vidc_relu_backward(const float* dy, const float* y, float* dx, long long M, int C, int lddy, int ldy, int lddx, int accumulate,
                                  vidc_stream_t stream) {
    VIDC_REQUIRE(dy && dx, VIDC_ERR_NULL, "vidc_relu_backward: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && (!y || ldy % 4 == 0), VIDC_ERR_SHAPE, "vidc_relu_backward: bad shape");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks(M * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), dy, y, dx, M, C, lddy, ldy, lddx, accumulate);
    VIDC_CHECK_LAUNCH("relu_bwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_maxpool3x3s2_backward(const float* x, const float* dy, float* dx, int B, int H, int W, int C, int ldx, int lddy, int lddx,
                                          vidc_stream_t stream) {
    VIDC_REQUIRE(x && dy && dx, VIDC_ERR_NULL, "vidc_maxpool3x3s2_backward: null pointer");
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, VIDC_ERR_SHAPE, "vidc_maxpool3x3s2_backward: bad shape");
    const long long Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;      // (the wide kernel indexes x, dx AND dy with 32-bit offsets)
    const bool wide = C % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && (long long)B * H * W * (ldx > lddx ? ldx : lddx) < (1ll << 31) &&
                      (long long)B * Ho * Wo * lddy < (1ll << 31) &&
                      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    if (wide)
        hipLaunchKernelGGL(maxpool_bwd_kernel<4>, dim3(blocks((long long)B * H * W * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), x, dy, dx, B, H, W, C, ldx, lddy, lddx);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<1>, dim3(blocks((long long)B * H * W * C)), dim3(TT), 0, vidc::as_stream(stream), x, dy, dx, B, H, W, C, ldx, lddy, lddx);
    VIDC_CHECK_LAUNCH("maxpool_bwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_upsample_bilinear_ac_backward(const float* dy, float* dx, int B, int h, int w, int C, int lddy, int lddx, int H, int W,
                                                  vidc_stream_t stream) {
    VIDC_REQUIRE(dy && dx, VIDC_ERR_NULL, "vidc_upsample_bilinear_ac_backward: null pointer");
    VIDC_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, VIDC_ERR_SHAPE, "vidc_upsample_bilinear_ac_backward: bad shape");
    const bool wide = C % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && (long long)B * H * W * lddy < (1ll << 31) && (long long)B * h * w * lddx < (1ll << 31) &&
                      ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    if (wide)
        hipLaunchKernelGGL(upsample_bwd_kernel<4>, dim3(blocks((long long)B * h * w * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), dy, dx, B, h, w, C, lddy, lddx, H, W);
    else
        hipLaunchKernelGGL(upsample_bwd_kernel<1>, dim3(blocks((long long)B * h * w * C)), dim3(TT), 0, vidc::as_stream(stream), dy, dx, B, h, w, C, lddy, lddx, H, W);
    VIDC_CHECK_LAUNCH("upsample_bwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_avgpool2d_backward(const float* dy, float* dx, int B, int H, int W, int C, int ldx, int kh, int kw, int sh, int sw, int ph, int pw,
                                       int ldy, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && dx, VIDC_ERR_NULL, "vidc_avgpool2d_backward: null pointer");
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C && kh > 0 && kw > 0 && sh > 0 && sw > 0 &&
                     ph >= 0 && pw >= 0 && (long long)H + 2ll * ph >= kh && (long long)W + 2ll * pw >= kw && (long long)H + ph < (1ll << 30) &&
                     (long long)W + pw < (1ll << 30) && (long long)kh * kw < (1ll << 24) && (long long)B * H < (1ll << 31),
                 VIDC_ERR_SHAPE, "vidc_avgpool2d_backward: bad shape (as vidc_avgpool2d; C, ldx, ldy multiples of 4)");
    VIDC_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0, VIDC_ERR_SHAPE,
                 "vidc_avgpool2d_backward: dy and dx must be 16-byte aligned");
    const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
    VIDC_REQUIRE((long long)B * Ho < (1ll << 31), VIDC_ERR_SHAPE, "vidc_avgpool2d_backward: bad shape");
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(blocks((long long)B * H * W * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), dy, dx, B, H, W, C, ldx, kh, kw,
                       sh, sw, ph, pw, Ho, Wo, ldy);
    VIDC_CHECK_LAUNCH("avgpool_bwd_kernel");
    return VIDC_OK;
}

extern "C" size_t vidc_head_backward_multi_scratch_bytes(int B, int h, int w, int C, int Cout, int pad) {
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || Cout <= 0 || pad < 0) return 0;
    const long long M = (long long)B * h * w, n = (long long)B * (h + 2 * pad) * (w + 2 * pad);
    return ((size_t)chunks_for(M) * Cout * C + (size_t)Cout * sum_blocks(n) + 8) * sizeof(double);
}

extern "C" int vidc_head_backward_multi(const float* g_low, const float* x, const float* wgt, float* dx, float* dw, float* dbias, int B, int h, int w, int C,
                                        int ldx, int lddx, int Cout, int pad, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(g_low && x && wgt && dx && dw && dbias && scratch, VIDC_ERR_NULL, "vidc_head_backward_multi: null pointer");
    VIDC_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && ldx >= C && lddx >= C && pad >= 0, VIDC_ERR_SHAPE, "vidc_head_backward_multi: bad shape");
    VIDC_REQUIRE(Cout >= 1 && Cout <= kMaxCout, VIDC_ERR_SHAPE, "vidc_head_backward_multi: Cout must be 1..4 (as vidc_head_conv1x1_upsample)");
    VIDC_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, VIDC_ERR_SHAPE, "vidc_head_backward_multi: scratch must be 8-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    const long long M = (long long)B * h * w;
    const long long plane = (long long)(h + 2 * pad) * (w + 2 * pad);
    const int nch = chunks_for(M), nb = sum_blocks((long long)B * plane), n_out = Cout * C;
    double* partial = reinterpret_cast<double*>(scratch);
    double* p2 = partial + (size_t)nch * n_out;
    hipLaunchKernelGGL(head_dgrad_kernel, dim3(blocks(M * C)), dim3(TT), 0, st, g_low, wgt, dx, B, h, w, C, Cout, pad, lddx);
    hipLaunchKernelGGL(head_wgrad_partial_kernel, dim3(blocks(C), nch), dim3(TT), 0, st, g_low, x, B, h, w, C, Cout, pad, ldx, partial);
    hipLaunchKernelGGL(head_wgrad_final_kernel, dim3((n_out + TT / kFinalLanes - 1) / (TT / kFinalLanes)), dim3(TT), 0, st, partial, nch, n_out, dw);
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nb, Cout), dim3(TT), 0, st, g_low, B, Cout, plane, p2);
    hipLaunchKernelGGL(sum_final_kernel, dim3(Cout), dim3(TT), 0, st, p2, nb, (double*)nullptr, dbias);
    VIDC_CHECK_LAUNCH("head_backward_multi");
    return VIDC_OK;
}

// the depth network's head: one output channel, pad 1
extern "C" size_t vidc_head_backward_scratch_bytes(int B, int h, int w, int C) { return vidc_head_backward_multi_scratch_bytes(B, h, w, C, 1, 1); }

extern "C" int vidc_head_backward(const float* g_low, const float* x, const float* wgt, float* dx, float* dw, float* dbias, int B, int h, int w, int C,
                                  int ldx, int lddx, void* scratch, vidc_stream_t stream) {
    return vidc_head_backward_multi(g_low, x, wgt, dx, dw, dbias, B, h, w, C, ldx, lddx, 1, 1, scratch, stream);
}

extern "C" int vidc_masked_l1_loss(const float* pred, const float* gt, long long n, int hw, double* loss, float* dpred, float* terms, void* scratch,
                                   vidc_stream_t stream) {
    VIDC_REQUIRE(pred && gt && loss && dpred && terms && scratch, VIDC_ERR_NULL, "vidc_masked_l1_loss: null pointer");
    VIDC_REQUIRE(n > 0 && hw > 0, VIDC_ERR_SHAPE, "vidc_masked_l1_loss: bad shape");
    hipStream_t st = vidc::as_stream(stream);
    hipLaunchKernelGGL(l1_loss_kernel, dim3(blocks(n)), dim3(TT), 0, st, pred, gt, n, 1.0f / (float)hw, terms, dpred);
    const int nb = sum_blocks(n);
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(TT), 0, st, terms, 1, 1, n, reinterpret_cast<double*>(scratch));
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(TT), 0, st, reinterpret_cast<const double*>(scratch), nb, loss, (float*)nullptr);
    VIDC_CHECK_LAUNCH("masked_l1_loss");
    return VIDC_OK;
}

extern "C" int vidc_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
                              vidc_stream_t stream) {
    VIDC_REQUIRE(p && g && m && v, VIDC_ERR_NULL, "vidc_adam_step: null pointer");
    VIDC_REQUIRE(n > 0 && step >= 1, VIDC_ERR_SHAPE, "vidc_adam_step: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    VIDC_REQUIRE(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0,
                 VIDC_ERR_SHAPE, "vidc_adam_step: the four buffers must be 16-byte aligned");
    hipLaunchKernelGGL(adam_kernel, dim3(blocks((n + 3) / 4)), dim3(TT), 0, vidc::as_stream(stream), p, g, m, v, n, lr, beta1, beta2, eps, (float)bc1,
                       (float)sqrt(bc2));
    VIDC_CHECK_LAUNCH("adam_kernel");
    return VIDC_OK;
}

// Gradient buckets in bf16 for the cross-rank SUM (training.GradientBuckets, VIDC_TRAIN_GRAD_BF16=1): 8 values per lane, 32 B in / 16 B out
// (narrow) and back; HBM-bound, one pass each.
__global__ void __launch_bounds__(TT) grad_narrow_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, long long n) {
    const long long i = ((long long)blockIdx.x * TT + threadIdx.x) * 8;
    if (i + 8 <= n) {
        float v[8];
        vidc::load4(x + i, v);
        vidc::load4(x + i + 4, v + 4);
        vidc::store8_bf16(y + i, v);
    } else {
        for (long long j = i; j < n; ++j) y[j] = vidc::bf16_rne(x[j]);
    }
}

__global__ void __launch_bounds__(TT) grad_widen_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, long long n) {
    const long long i = ((long long)blockIdx.x * TT + threadIdx.x) * 8;
    if (i + 8 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + i);
        *reinterpret_cast<float4*>(y + i) = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u));
        *reinterpret_cast<float4*>(y + i + 4) = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xFFFF0000u), __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xFFFF0000u));
    } else {
        for (long long j = i; j < n; ++j) y[j] = __uint_as_float((unsigned)x[j] << 16);
    }
}

extern "C" int vidc_grad_narrow_bf16(const float* x, void* y_bf16, long long n, vidc_stream_t stream) {
    VIDC_REQUIRE(x && y_bf16, VIDC_ERR_NULL, "vidc_grad_narrow_bf16: null pointer");
    VIDC_REQUIRE(n > 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y_bf16 % 16) == 0, VIDC_ERR_SHAPE, "vidc_grad_narrow_bf16: n > 0 and 16-byte aligned buffers");
    hipLaunchKernelGGL(grad_narrow_kernel, dim3((unsigned)((n + (long long)TT * 8 - 1) / ((long long)TT * 8))), dim3(TT), 0, vidc::as_stream(stream), x,
                       reinterpret_cast<unsigned short*>(y_bf16), n);
    VIDC_CHECK_LAUNCH("grad_narrow_kernel");
    return VIDC_OK;
}

extern "C" int vidc_grad_widen_bf16(const void* x_bf16, float* y, long long n, vidc_stream_t stream) {
    VIDC_REQUIRE(x_bf16 && y, VIDC_ERR_NULL, "vidc_grad_widen_bf16: null pointer");
    VIDC_REQUIRE(n > 0 && ((uintptr_t)x_bf16 % 16) == 0 && ((uintptr_t)y % 16) == 0, VIDC_ERR_SHAPE, "vidc_grad_widen_bf16: n > 0 and 16-byte aligned buffers");
    hipLaunchKernelGGL(grad_widen_kernel, dim3((unsigned)((n + (long long)TT * 8 - 1) / ((long long)TT * 8))), dim3(TT), 0, vidc::as_stream(stream),
                       reinterpret_cast<const unsigned short*>(x_bf16), y, n);
    VIDC_CHECK_LAUNCH("grad_widen_kernel");
    return VIDC_OK;
}

extern "C" int vidc_pack_conv_weight_dgrad(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, vidc_stream_t stream) {
    VIDC_REQUIRE(w_oihw && w_packed, VIDC_ERR_NULL, "vidc_pack_conv_weight_dgrad: null pointer");
    VIDC_REQUIRE(Cout > 0 && Cout % 32 == 0 && Cin > 0 && KH > 0 && KW > 0, VIDC_ERR_SHAPE, "vidc_pack_conv_weight_dgrad: Cout must be a multiple of 32");
    const long long total = (long long)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(pack_weight_dgrad_kernel, dim3(blocks(total)), dim3(TT), 0, vidc::as_stream(stream), w_oihw, w_packed, Cout, Cin, KH, KW);
    VIDC_CHECK_LAUNCH("pack_weight_dgrad_kernel");
    return VIDC_OK;
}

extern "C" long long vidc_pack_item_blocks(int Cout, int Cin, int KH, int KW, int kind) {
    if (Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || KH * KW > 9 || kind < 0 || kind > 5) return 0;
    const int U = (kind & 4) ? 64 : 32;
    if (((kind & 1) ? Cout : Cin) % U) return 0;          // the K-side channel count must fill whole 128-byte units
    return pack_item_blocks(Cout, Cin, KH, KW, kind);
}

extern "C" int vidc_pack_conv_weights_batched(const vidc_pack_item* items_device, int n_items, long long total_blocks, vidc_stream_t stream) {
    VIDC_REQUIRE(items_device, VIDC_ERR_NULL, "vidc_pack_conv_weights_batched: null pointer");
    VIDC_REQUIRE(n_items > 0 && total_blocks > 0 && total_blocks < (1ll << 31), VIDC_ERR_SHAPE, "vidc_pack_conv_weights_batched: bad item / block count");
    hipLaunchKernelGGL(pack_batched_kernel, dim3((unsigned)total_blocks), dim3(TT), 0, vidc::as_stream(stream), items_device, n_items);
    VIDC_CHECK_LAUNCH("pack_batched_kernel");
    return VIDC_OK;
}

extern "C" int vidc_pack_conv_weights_one(const float* w_oihw, void* packed, int Cout, int Cin, int KH, int KW, int kind, vidc_stream_t stream) {
    VIDC_REQUIRE(w_oihw && packed, VIDC_ERR_NULL, "vidc_pack_conv_weights_one: null pointer");
    const long long nb = vidc_pack_item_blocks(Cout, Cin, KH, KW, kind);
    VIDC_REQUIRE(nb > 0 && nb < (1ll << 31), VIDC_ERR_SHAPE, "vidc_pack_conv_weights_one: %dx%dx%dx%d cannot be packed as kind %d", Cout, Cin, KH, KW, kind);
    vidc_pack_item it = {};
    it.w = w_oihw;
    it.packed = reinterpret_cast<float*>(packed);
    it.Cout = Cout; it.Cin = Cin; it.KH = KH; it.KW = KW;
    it.kind = kind;
    it.block_begin = 0;
    hipLaunchKernelGGL(pack_one_kernel, dim3((unsigned)nb), dim3(TT), 0, vidc::as_stream(stream), it);
    VIDC_CHECK_LAUNCH("pack_one_kernel");
    return VIDC_OK;
}

extern "C" int vidc_cast_bf16(const float* x, void* y, long long rows, int C, int ldx, vidc_stream_t stream) {
    VIDC_REQUIRE(x && y, VIDC_ERR_NULL, "vidc_cast_bf16: null pointer");
    VIDC_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && ldx >= C && ldx % 4 == 0, VIDC_ERR_SHAPE, "vidc_cast_bf16: C must be a multiple of 8");
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks(rows * (C / 8))), dim3(TT), 0, vidc::as_stream(stream), x, reinterpret_cast<unsigned short*>(y), rows, C, ldx);
    VIDC_CHECK_LAUNCH("cast_bf16_kernel");
    return VIDC_OK;
}

extern "C" int vidc_zero_stuff(const float* dy, float* z, int B, int Ho, int Wo, int C, int lddy, int stride, int H, int W, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && z, VIDC_ERR_NULL, "vidc_zero_stuff: null pointer");
    VIDC_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && lddy % 4 == 0 && stride >= 1 && (Ho - 1) * stride < H && (Wo - 1) * stride < W,
                 VIDC_ERR_SHAPE, "vidc_zero_stuff: bad shape");
    hipLaunchKernelGGL(zero_stuff_kernel, dim3(blocks((long long)B * H * W * (C / 4))), dim3(TT), 0, vidc::as_stream(stream), dy, z, B, Ho, Wo, C, lddy,
                       stride, H, W);
    VIDC_CHECK_LAUNCH("zero_stuff_kernel");
    return VIDC_OK;
}

void vidc::launch_wgrad_final(const float* partial, int chunks, int taps, int Cout, int Cin, float* dw_oihw, hipStream_t st) {
    hipLaunchKernelGGL(wgrad_final_kernel, dim3(blocks((long long)taps * Cout * Cin)), dim3(TT), 0, st, partial, chunks, taps, Cout, Cin, dw_oihw);
}

namespace {
inline int wgrad_rows_per_chunk(long long M, int Cout, int Cin, int taps) {
    // enough workgroups to fill 256 CUs, chunks of at least 256 pixels (a multiple of 16)
    const long long tiles = (long long)((Cout + 127) / 128) * ((Cin + 127) / 128) * taps;
    long long chunks = (1024 + tiles - 1) / tiles;
    if (chunks < 1) chunks = 1;
    long long rows = (M + chunks - 1) / chunks;
    if (rows < 256) rows = 256;
    if (rows > 1024) rows = 1024;       // short fp32 accumulation chains (the partials are then summed in fp64): keeps dW within ~1e-4 of an
    rows = (rows + 7) / 8 * 8;          // fp64 evaluation even where the sum over 10^4..10^5 pixels cancels heavily
    return (int)rows;
}
}

extern "C" size_t vidc_conv_wgrad_scratch_bytes(int B, int Ho, int Wo, int Cout, int Cin, int KH, int KW) {
    const long long M = (long long)B * Ho * Wo;
    const int rows = wgrad_rows_per_chunk(M, Cout, Cin, KH * KW);
    const long long chunks = (M + rows - 1) / rows;
    return (size_t)chunks * KH * KW * (size_t)Cout * Cin * sizeof(float);
}

namespace {
// vidc_conv_wgrad and vidc_conv_wgrad_dilated: one body, one kernel; dilation 1 launches exactly what the plain entry always launched.
int conv_wgrad_launch(const char* what, const float* dy, const float* x, float* dw_oihw, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout,
                      int lddy, int KH, int KW, int stride, int pad, int dilation, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && x && dw_oihw && scratch, VIDC_ERR_NULL, "%s: null pointer", what);
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && dilation >= 1 && ldx >= Cin && lddy >= Cout,
                 VIDC_ERR_SHAPE, "%s: bad shape", what);
    VIDC_REQUIRE((long long)dilation * (KH - 1) <= H + 2 * pad - 1 && (long long)dilation * (KW - 1) <= W + 2 * pad - 1 &&
                     Ho == (H + 2 * pad - dilation * (KH - 1) - 1) / stride + 1 && Wo == (W + 2 * pad - dilation * (KW - 1) - 1) / stride + 1,
                 VIDC_ERR_SHAPE, "%s: Ho/Wo inconsistent", what);
    VIDC_REQUIRE((long long)B * H * W * ldx < (1ll << 31) && (long long)B * Ho * Wo * lddy < (1ll << 31), VIDC_ERR_SHAPE,
                 "%s: tensors must stay below 2^31 elements (32-bit offsets)", what);
    hipStream_t st = vidc::as_stream(stream);
    const long long M = (long long)B * Ho * Wo;
    const int taps = KH * KW;
    const int rows = wgrad_rows_per_chunk(M, Cout, Cin, taps);
    const int chunks = (int)((M + rows - 1) / rows);
    float* partial = reinterpret_cast<float*>(scratch);
    hipLaunchKernelGGL(wgrad_kernel, dim3((Cout + 127) / 128, ((Cin + 127) / 128) * taps, chunks), dim3(256), 0, st, dy, x, B, H, W, Cin, ldx, Ho, Wo, Cout, lddy,
                       KH, KW, stride, pad, dilation, rows, partial);
    vidc::launch_wgrad_final(partial, chunks, taps, Cout, Cin, dw_oihw, st);
    VIDC_CHECK_LAUNCH("conv_wgrad");
    return VIDC_OK;
}
}

extern "C" int vidc_conv_wgrad(const float* dy, const float* x, float* dw_oihw, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int lddy,
                               int KH, int KW, int stride, int pad, void* scratch, vidc_stream_t stream) {
    return conv_wgrad_launch("vidc_conv_wgrad", dy, x, dw_oihw, B, H, W, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad, 1, scratch, stream);
}

// (the scratch does not depend on the dilation: the partials are [chunk][tap][Cout][Cin] of the same output pixels)
extern "C" size_t vidc_conv_wgrad_dilated_scratch_bytes(int B, int Ho, int Wo, int Cout, int Cin, int KH, int KW) {
    return vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, Cout, Cin, KH, KW);
}

extern "C" int vidc_conv_wgrad_dilated(const float* dy, const float* x, float* dw_oihw, int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int lddy,
                                       int KH, int KW, int stride, int pad, int dilation, void* scratch, vidc_stream_t stream) {
    return conv_wgrad_launch("vidc_conv_wgrad_dilated", dy, x, dw_oihw, B, H, W, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad, dilation, scratch, stream);
}

namespace {
// vidc_im2col_transposed and vidc_im2col_transposed_dilated: one body, the same two kernels.
int im2col_transposed_launch(const char* what, const float* x, float* xt, int B, int H, int W, int C, int ldx, int Ho, int Wo, int KH, int KW, int stride,
                             int pad, int dilation, int Mp, int split, vidc_stream_t stream) {
    VIDC_REQUIRE(x && xt, VIDC_ERR_NULL, "%s: null pointer", what);
    const long long M = (long long)B * Ho * Wo;
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && dilation >= 1 && Mp >= M &&
                     Mp % 32 == 0 && M < (1ll << 31) && (long long)KH * KW <= 65535 && split >= 0 && (split & 3) <= 2 && split < 8 && ((split & 3) != 2 || Mp % 64 == 0),
                 VIDC_ERR_SHAPE, "%s: bad shape (Mp = M rounded up to a multiple of 32; 64 for plain bf16 rows)", what);
    // (a tap's coordinate stays an int: the kernels test it against the image before they form an address)
    VIDC_REQUIRE((long long)(Ho - 1) * stride + (long long)(KH - 1) * dilation < (1ll << 30) && (long long)(Wo - 1) * stride + (long long)(KW - 1) * dilation < (1ll << 30),
                 VIDC_ERR_SHAPE, "%s: tap coordinates out of range", what);
    const bool wide = C % 4 == 0 && ldx % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xt)) & 15) == 0;
    if (wide)
        hipLaunchKernelGGL(im2col_t64_kernel<float>, dim3((Mp + 63) / 64, (C + 63) / 64, KH * KW), dim3(256), 0, vidc::as_stream(stream), x, xt, B, H, W, C, ldx, Ho, Wo,
                           KH, KW, stride, pad, dilation, (int)M, Mp, split);
    else
        hipLaunchKernelGGL(im2col_t_kernel, dim3(Mp / 32, (C + 31) / 32, KH * KW), dim3(256), 0, vidc::as_stream(stream), x, xt, B, H, W, C, ldx, Ho, Wo, KH, KW,
                           stride, pad, dilation, (int)M, Mp, split);
    VIDC_CHECK_LAUNCH("im2col_t_kernel");
    return VIDC_OK;
}
}

extern "C" int vidc_im2col_transposed(const float* x, float* xt, int B, int H, int W, int C, int ldx, int Ho, int Wo, int KH, int KW, int stride, int pad,
                                      int Mp, int split, vidc_stream_t stream) {
    return im2col_transposed_launch("vidc_im2col_transposed", x, xt, B, H, W, C, ldx, Ho, Wo, KH, KW, stride, pad, 1, Mp, split, stream);
}

extern "C" int vidc_im2col_transposed_dilated(const float* x, float* xt, int B, int H, int W, int C, int ldx, int Ho, int Wo, int KH, int KW, int stride, int pad,
                                              int dilation, int Mp, int split, vidc_stream_t stream) {
    return im2col_transposed_launch("vidc_im2col_transposed_dilated", x, xt, B, H, W, C, ldx, Ho, Wo, KH, KW, stride, pad, dilation, Mp, split, stream);
}

extern "C" int vidc_im2col_transposed_bf16(const void* x_bf16, void* xt_bf16, int B, int H, int W, int C, int Ho, int Wo, int KH, int KW, int stride, int pad,
                                           int Mp, vidc_stream_t stream) {
    VIDC_REQUIRE(x_bf16 && xt_bf16, VIDC_ERR_NULL, "vidc_im2col_transposed_bf16: null pointer");
    const long long M = (long long)B * Ho * Wo;
    VIDC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && Mp >= M && Mp % 64 == 0 && M < (1ll << 31) &&
                     (long long)B * H * W * C < (1ll << 31) && (long long)KH * KW <= 65535 &&
                     ((reinterpret_cast<uintptr_t>(x_bf16) | reinterpret_cast<uintptr_t>(xt_bf16)) & 7) == 0,
                 VIDC_ERR_SHAPE, "vidc_im2col_transposed_bf16: bad shape (C a multiple of 4, Mp = M rounded up to a multiple of 64, 8-byte aligned tensors)");
    // (dense rows, no dilation; 4 | 2: channel-major rows of plain bf16)
    hipLaunchKernelGGL(im2col_t64_kernel<unsigned short>, dim3(Mp / 64, (C + 63) / 64, KH * KW), dim3(256), 0, vidc::as_stream(stream),
                       reinterpret_cast<const unsigned short*>(x_bf16), reinterpret_cast<unsigned short*>(xt_bf16), B, H, W, C, C, Ho, Wo, KH, KW, stride, pad, 1,
                       (int)M, Mp, 4 | 2);
    VIDC_CHECK_LAUNCH("im2col_t64_kernel<unsigned short>");
    return VIDC_OK;
}

extern "C" int vidc_transpose_bf16(const void* x_bf16, void* xt_bf16, long long M, int C, int Mp, vidc_stream_t stream) {
    VIDC_REQUIRE(x_bf16 && xt_bf16, VIDC_ERR_NULL, "vidc_transpose_bf16: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 8 == 0 && Mp >= M && Mp % 64 == 0 && M < (1ll << 31) &&
                     ((reinterpret_cast<uintptr_t>(x_bf16) | reinterpret_cast<uintptr_t>(xt_bf16)) & 15) == 0,
                 VIDC_ERR_SHAPE, "vidc_transpose_bf16: C a multiple of 8, Mp = M rounded up to a multiple of 64, 16-byte aligned tensors");
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3(Mp / 64, (C + 63) / 64), dim3(256), 0, vidc::as_stream(stream),
                       reinterpret_cast<const unsigned short*>(x_bf16), reinterpret_cast<unsigned short*>(xt_bf16), (int)M, C, Mp);
    VIDC_CHECK_LAUNCH("transpose_bf16_kernel");
    return VIDC_OK;
}

extern "C" int vidc_wgrad_permute(const float* tmp, float* dw_oihw, int Cout, int Cin, int taps, vidc_stream_t stream) {
    VIDC_REQUIRE(tmp && dw_oihw, VIDC_ERR_NULL, "vidc_wgrad_permute: null pointer");
    VIDC_REQUIRE(Cout > 0 && Cin > 0 && taps > 0, VIDC_ERR_SHAPE, "vidc_wgrad_permute: bad shape");
    hipLaunchKernelGGL(wgrad_permute_kernel, dim3(blocks((long long)Cout * Cin * taps)), dim3(TT), 0, vidc::as_stream(stream), tmp, dw_oihw, Cout, Cin, taps);
    VIDC_CHECK_LAUNCH("wgrad_permute_kernel");
    return VIDC_OK;
}

extern "C" int vidc_stem_wgrad(const float* dy, const float* x_nchw, float* dw_oihw, int B, int Cin, int H, int W, int Cout, int lddy, void* scratch,
                               vidc_stream_t stream) {
    VIDC_REQUIRE(dy && x_nchw && dw_oihw && scratch, VIDC_ERR_NULL, "vidc_stem_wgrad: null pointer");
    VIDC_REQUIRE(B > 0 && Cin > 0 && Cin <= 4 && H > 0 && W > 0 && Cout > 0 && lddy >= Cout, VIDC_ERR_SHAPE, "vidc_stem_wgrad: bad shape");
    hipStream_t st = vidc::as_stream(stream);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long M = (long long)B * Ho * Wo;
    const int n = Cout * Cin * 9;
    const int rows = kStemRows;
    const int chunks = (int)((M + rows - 1) / rows);
    double* partial = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(stem_wgrad_partial_kernel, dim3(blocks((long long)Cout * Cin), chunks), dim3(TT), 0, st, dy, x_nchw, B, Cin, H, W, Ho, Wo, Cout, lddy, rows, partial);
    hipLaunchKernelGGL(head_wgrad_final_kernel, dim3((n + TT / kFinalLanes - 1) / (TT / kFinalLanes)), dim3(TT), 0, st, partial, chunks, n, dw_oihw);
    VIDC_CHECK_LAUNCH("stem_wgrad");
    return VIDC_OK;
}

extern "C" size_t vidc_stem_wgrad_scratch_bytes(int B, int Cin, int H, int W, int Cout) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long M = (long long)B * Ho * Wo;
    return (size_t)((M + kStemRows - 1) / kStemRows) * (size_t)Cout * Cin * 9 * sizeof(double);
}

// ---- backward of the per-op surface (torch.ops.vidc.*, torch_ops.py) ------------------------------------------------------------------------
namespace {

// The epilogue of vidc_conv2d_bn_act, y = relu?(c * scale + shift), transposed in one pass over the NHWC rows: dc = mask(dy) * scale (the operand
// of dgrad and wgrad) and the chunk sums of mask(dy) and mask(dy) * c in fp64, c = (y - shift) / scale -- where the mask is open y determines c,
// where it is closed the term is zero.  A channel with scale == 0 reads c from `craw` (the conv re-run with an identity epilogue; the caller
// passes it only when such a channel exists), with all_raw every channel does (a forward whose y is not an fp32-accurate image of c).
// So does, when craw is given, an ill-conditioned channel: |shift| > kAffineIllCond * |scale|.  y = fl(c * scale + shift) carries an absolute
// error of up to u * max(|c * scale|, |shift|), so the quotient returns c with an error of up to ~u * (|c| + |shift / scale|): at most
// u * (|c| + kAffineIllCond) where the rule reconstructs -- for a conv output of the order of 1 that is below the rounding the fp32 conv
// itself leaves in c (the rule reads scale and shift alone and so assumes that order) -- and without bound where it does not (scale 2^-10,
// shift 1: dscale off by 1e-5 of its size; scale 1e-30: y == shift in every row and dscale == 0).  The threshold is a power of two, so
// kAffineIllCond * |scale| is the same fp32 value on the host (torch_ops._conv_backward_body decides there whether the conv is re-run) and
// here, and a channel the rule keeps is computed exactly as in a call without craw: same bits.
// Block / grid / summation order: chan_partial_kernel's.
constexpr float kAffineIllCond = 4.f;       // torch_ops.AFFINE_ILL_COND
__global__ void __launch_bounds__(TT)
affine_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ craw, const float* __restrict__ scale,
                      const float* __restrict__ shift, float* __restrict__ dc, long long M, int C, int lddy, int ldy, int ldc, int lddc, int relu,
                      int all_raw, int rows_per_chunk, double* __restrict__ partial) {
    __shared__ double red[2][16][64];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + cq * 4;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    if (c < C) {
        float sc[4], sh[4];
        bool raw[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sc[k] = scale[c + k];
            sh[k] = shift[c + k];
            raw[k] = all_raw || sc[k] == 0.f || (craw && fabsf(sh[k]) > kAffineIllCond * fabsf(sc[k]));
        }
        for (long long r = r0 + rl; r < r1; r += 16) {
            const float4 gv = *reinterpret_cast<const float4*>(dy + r * lddy + c);
            const float4 yv4 = *reinterpret_cast<const float4*>(y + r * ldy + c);
            float g[4] = {gv.x, gv.y, gv.z, gv.w};
            const float yv[4] = {yv4.x, yv4.y, yv4.z, yv4.w};
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (relu && !(yv[k] > 0.f)) g[k] = 0.f;
                float cv;
                if (!raw[k]) cv = (yv[k] - sh[k]) / sc[k];
                else cv = craw ? craw[r * ldc + c + k] : 0.f;
                s0[k] += (double)g[k];
                s1[k] += (double)g[k] * (double)cv;
                o[k] = g[k] * sc[k];
            }
            *reinterpret_cast<float4*>(dc + r * lddc + c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[0][rl][cq * 4 + k] = s0[k]; red[1][rl][cq * 4 + k] = s1[k]; }
    __syncthreads();
    if (threadIdx.x < 128) {                       // 64 channels x 2 sums; row-lanes added in order 0..15
        const int q = threadIdx.x >> 6, l = threadIdx.x & 63, cc = blockIdx.x * 64 + l;
        if (cc < C) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) t += red[q][j][l];
            partial[((size_t)blockIdx.y * 2 + q) * C + cc] = t;
        }
    }
}

// dx (NCHW) of the 3x3 / stride-2 / pad-1 stem conv, gather form: one thread per input pixel and all Cin channels; the up to 2 x 2 output pixels
// whose window holds it are read as NHWC rows (ReLU mask from y), the weights from LDS as [tap][ci][co].  Fixed order (ky, kx, co): reproducible.
__global__ void __launch_bounds__(256)
stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w_oihw, float* __restrict__ dx, int B, int Cin,
                  int H, int W, int Ho, int Wo, int Cout, int lddy, int ldy) {
    extern __shared__ float ws[];
    for (int i = threadIdx.x; i < Cout * Cin * 9; i += blockDim.x) {
        const int co = i / (Cin * 9), r = i - co * (Cin * 9), ci = r / 9, t = r - ci * 9;
        ws[(t * Cin + ci) * Cout + co] = w_oihw[i];
    }
    __syncthreads();
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * H * W) return;
    const int ix = (int)(idx % W), iy = (int)((idx / W) % H), b = (int)(idx / ((long long)W * H));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 3; ++ky) {
        const int ty = iy + 1 - ky;
        if (ty < 0 || (ty & 1) || (ty >> 1) >= Ho) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int tx = ix + 1 - kx;
            if (tx < 0 || (tx & 1) || (tx >> 1) >= Wo) continue;
            const size_t row = ((size_t)b * Ho + (ty >> 1)) * Wo + (tx >> 1);
            const float* g = dy + row * lddy;
            const float* yy = y ? y + row * ldy : nullptr;
            const float* wt = ws + (size_t)(ky * 3 + kx) * Cin * Cout;
            for (int co = 0; co < Cout; co += 4) {
                float4 gv = *reinterpret_cast<const float4*>(g + co);
                if (yy) {
                    const float4 yv = *reinterpret_cast<const float4*>(yy + co);
                    if (!(yv.x > 0.f)) gv.x = 0.f;
                    if (!(yv.y > 0.f)) gv.y = 0.f;
                    if (!(yv.z > 0.f)) gv.z = 0.f;
                    if (!(yv.w > 0.f)) gv.w = 0.f;
                }
                for (int ci = 0; ci < Cin; ++ci) {
                    const float* wc = wt + ci * Cout + co;
                    acc[ci] = fmaf(gv.w, wc[3], fmaf(gv.z, wc[2], fmaf(gv.y, wc[1], fmaf(gv.x, wc[0], acc[ci]))));
                }
            }
        }
    }
    const size_t plane = (size_t)H * W;
    float* o = dx + (size_t)b * Cin * plane + (size_t)iy * W + ix;
    for (int ci = 0; ci < Cin; ++ci) o[ci * plane] = acc[ci];
}

}  // namespace

extern "C" int vidc_affine_act_backward(const float* dy, const float* y, const float* c_raw, const float* scale, const float* shift, float* dc,
                                        float* dscale, float* dshift, long long M, int C, int lddy, int ldy, int ldc, int lddc, int relu, void* scratch,
                                        vidc_stream_t stream) {
    VIDC_REQUIRE(dy && y && scale && shift && dc && dscale && dshift && scratch, VIDC_ERR_NULL, "vidc_affine_act_backward: null pointer");
    VIDC_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && lddy >= C && ldy >= C && lddc >= C && lddy % 4 == 0 && ldy % 4 == 0 && lddc % 4 == 0 &&
                 (!c_raw || ldc >= C || -ldc >= C), VIDC_ERR_SHAPE, "vidc_affine_act_backward: bad shape (C and the row strides multiples of 4)");
    VIDC_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dc)) & 15) == 0, VIDC_ERR_SHAPE,
                 "vidc_affine_act_backward: dy, y and dc must be 16-byte aligned");
    hipStream_t st = vidc::as_stream(stream);
    const int nch = chunks_for(M, C);
    double* partial = reinterpret_cast<double*>(scratch);
    double* sums = partial + (size_t)nch * 2 * C;
    hipLaunchKernelGGL(affine_act_bwd_kernel, dim3((C + 63) / 64, nch), dim3(TT), 0, st, dy, y, c_raw, scale, shift, dc, M, C, lddy, ldy,
                       ldc < 0 ? -ldc : ldc, lddc, relu, (c_raw && ldc < 0) ? 1 : 0, rows_for(M, C), partial);
    hipLaunchKernelGGL(chan_final_kernel<FinalParamGrad>, dim3((C + 7) / 8), dim3(TT), 0, st, partial, nch, C, sums, FinalParamGrad{dscale, dshift});
    VIDC_CHECK_LAUNCH("affine_act_backward");
    return VIDC_OK;
}

extern "C" int vidc_stem_conv3x3s2_backward_data(const float* dy, const float* y_relu, const float* w_oihw, float* dx_nchw, int B, int Cin, int H, int W,
                                                 int Cout, int lddy, int ldy, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && w_oihw && dx_nchw, VIDC_ERR_NULL, "vidc_stem_conv3x3s2_backward_data: null pointer");
    VIDC_REQUIRE(B > 0 && Cin > 0 && Cin <= 4 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0 && lddy >= Cout && lddy % 4 == 0 &&
                 (!y_relu || (ldy >= Cout && ldy % 4 == 0)) && (size_t)Cout * Cin * 9 * sizeof(float) <= 48 * 1024, VIDC_ERR_SHAPE,
                 "vidc_stem_conv3x3s2_backward_data: bad shape (Cin <= 4, Cout and the row strides multiples of 4, weights within 48 KiB of LDS)");
    VIDC_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y_relu)) & 15) == 0, VIDC_ERR_SHAPE,
                 "vidc_stem_conv3x3s2_backward_data: dy and y must be 16-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(stem_dgrad_kernel, dim3(blocks((long long)B * H * W)), dim3(256), (size_t)Cout * Cin * 9 * sizeof(float), vidc::as_stream(stream), dy,
                       y_relu, w_oihw, dx_nchw, B, Cin, H, W, Ho, Wo, Cout, lddy, ldy);
    VIDC_CHECK_LAUNCH("stem_dgrad_kernel");
    return VIDC_OK;
}
