// The trainers' optimizer options on the device: Adam with weight decay (torch.optim.Adam's L2 form or torch.optim.AdamW's decoupled form),
// parameter groups (a learning-rate scale, a weight decay and a frozen flag per run of the flat buffer), the gradient's global norm with the
// clip factor of torch.nn.utils.clip_grad_norm_, and gradient accumulation over micro-steps.  All of it is passes over the flat parameter /
// gradient / moment buffers of training.py (HBM-bound: 4, 12 and 28 bytes per parameter); nothing is read back on the host.
//
// Segment table (how parameter groups reach the kernels): seg_begin[nseg + 1] int64, strictly increasing from 0 to n; seg_lr_scale[nseg],
// seg_weight_decay[nseg] float; seg_flags[nseg], bit 0 = frozen.  Boundaries fall anywhere: a thread whose four elements lie inside one
// segment uses 16-byte accesses as adam_kernel does, one that straddles a boundary (or the end of the buffer) goes element by element.  A
// workgroup finds the segment of its first element once (a 64-ary search by its first wave, broadcast through LDS); its threads walk on
// from there.
#include "common.h"
#include "optim.h"
#include <cstdint>

namespace {

using vidc::TT;
using vidc::blocks;
using vidc::block_tree;
using vidc::adam_one;

constexpr int kFrozen = 1;                           // seg_flags bit 0
constexpr int kNormPer = 8;                          // float4 loads per thread of sqnorm_partial_kernel
constexpr long long kNormChunk = (long long)TT * 4 * kNormPer;      // elements per workgroup of the norm pass (8192)

inline int norm_chunks(long long n) { return (int)((n + kNormChunk - 1) / kNormChunk); }

// The segment that holds element `start` (the largest s with seg_begin[s] <= start), found by the workgroup's first wave: every round its
// 64 lanes probe 64 evenly spaced boundaries of the remaining range and the count of those not beyond `start` narrows it 64-fold.
__device__ __forceinline__ int first_segment(const long long* __restrict__ seg_begin, int nseg, long long start, int* shared) {
    if (threadIdx.x < 64) {
        int lo = 0, hi = nseg;                       // invariant: seg_begin[lo] <= start < seg_begin[hi]
        while (hi - lo > 1) {
            const int step = (hi - lo + 63) / 64, idx = lo + (int)threadIdx.x * step;
            const bool le = idx < hi && seg_begin[idx] <= start;
            const int cnt = __popcll(__ballot(le));  // lane 0 always counts (the invariant), and the lanes that count form a prefix
            lo += (cnt - 1) * step;
            hi = min(hi, lo + step);
        }
        if (threadIdx.x == 0) *shared = lo;
    }
    __syncthreads();
    return *shared;
}

// ---- sum of squares of the non-frozen gradient, in fp64 ----------------------------------------------------------------------------------
// A square of an fp32 value is exact in fp64; the sums round.  Fixed order: a thread's values in ascending address order, block_tree, then
// the chunk partials by sqnorm_final_kernel -- two runs give the same bits.  No floating-point atomics.
__global__ void __launch_bounds__(TT)
sqnorm_partial_kernel(const float* __restrict__ g, long long n, int nseg, const long long* __restrict__ seg_begin, const int* __restrict__ seg_flags,
                      double* __restrict__ partial) {
    __shared__ double red[1][TT];
    __shared__ int s_first;
    const long long base = (long long)blockIdx.x * kNormChunk;
    int s = nseg > 0 ? first_segment(seg_begin, nseg, base, &s_first) : 0;
    double acc = 0.0;
    if (nseg == 0 && base + kNormChunk <= n) {       // a whole chunk, no table: the eight loads issued together, then the same sums in the same order
        float4 v[kNormPer];
#pragma unroll
        for (int k = 0; k < kNormPer; ++k) v[k] = *reinterpret_cast<const float4*>(g + base + ((long long)k * TT + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < kNormPer; ++k) {
            acc += (double)v[k].x * (double)v[k].x;
            acc += (double)v[k].y * (double)v[k].y;
            acc += (double)v[k].z * (double)v[k].z;
            acc += (double)v[k].w * (double)v[k].w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kNormPer; ++k) {
            const long long i = base + ((long long)k * TT + threadIdx.x) * 4;
            if (i >= n) break;
            bool whole = i + 4 <= n;
            if (nseg > 0) {
                while (seg_begin[s + 1] <= i) ++s;       // (i < n = seg_begin[nseg]: s stays below nseg)
                whole = whole && i + 4 <= seg_begin[s + 1];
            }
            if (whole) {
                if (nseg > 0 && (seg_flags[s] & kFrozen)) continue;
                const float4 v = *reinterpret_cast<const float4*>(g + i);
                acc += (double)v.x * (double)v.x;
                acc += (double)v.y * (double)v.y;
                acc += (double)v.z * (double)v.z;
                acc += (double)v.w * (double)v.w;
            } else {
                int t = s;
                for (long long e = i; e < n && e < i + 4; ++e) {
                    if (nseg > 0) {
                        while (seg_begin[t + 1] <= e) ++t;
                        if (seg_flags[t] & kFrozen) continue;
                    }
                    const double x = (double)g[e];
                    acc += x * x;
                }
            }
        }
    }
    red[0][threadIdx.x] = acc;
    block_tree<1>(red);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0][0];
}

// One workgroup: thread t adds partials t, t + TT, ... in order (eight loads in flight), block_tree, then the record:
// record[0] = grad_scale * sqrt(sum), record[1] = grad_scale * min(1, max_norm / (record[0] + 1e-6)) -- clip_grad_norm_'s total norm and
// clamped coefficient on the scaled gradient; max_norm <= 0: no clipping.  A non-finite norm propagates as it does in torch.
__global__ void __launch_bounds__(TT)
sqnorm_final_kernel(const double* __restrict__ partial, int nb, double grad_scale, double max_norm, double* __restrict__ record) {
    __shared__ double red[1][TT];
    double s = 0.0;
    for (int i0 = threadIdx.x; i0 < nb; i0 += TT * 8) {
        double u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * TT;
            u[j] = i < nb ? partial[i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += u[j];
    }
    red[0][threadIdx.x] = s;
    block_tree<1>(red);
    if (threadIdx.x == 0) {
        const double norm = grad_scale * sqrt(red[0][0]);
        double coef = 1.0;
        if (max_norm > 0.0) {
            const double c = max_norm / (norm + 1e-6);
            coef = c >= 1.0 ? 1.0 : c;               // (a NaN stays a NaN: torch.clamp(max=1.0))
        }
        record[0] = norm;
        record[1] = grad_scale * coef;
    }
}

// ---- gradient accumulation ---------------------------------------------------------------------------------------------------------------
// dst = src (first micro-step of a window) or dst += src: one fp32 add per element, 16-byte accesses, the n % 4 tail scalar
template <bool kFirst>
__global__ void __launch_bounds__(TT) accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n) {
    const long long i = ((long long)blockIdx.x * TT + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        float4 a = *reinterpret_cast<const float4*>(src + i);
        if (!kFirst) {
            const float4 d = *reinterpret_cast<const float4*>(dst + i);
            a = make_float4(d.x + a.x, d.y + a.y, d.z + a.z, d.w + a.w);
        }
        *reinterpret_cast<float4*>(dst + i) = a;
    } else {
        for (long long k = i; k < n; ++k) dst[k] = kFirst ? src[k] : dst[k] + src[k];
    }
}

// ---- the optimizer step ------------------------------------------------------------------------------------------------------------------
struct OptArgs {
    float lr, b1, b2, eps, bc1, bc2_sqrt, grad_scale;
    int decoupled, nseg;
    const double* record;
    const long long* seg_begin;
    const float *seg_lr_scale, *seg_weight_decay;
    const int* seg_flags;
};

// What a segment sets for its elements: step_size = lr_e / bc1 with lr_e = lr * lr_scale, the weight decay, and AdamW's factor
// 1 - lr_e * wd, rounded to fp32 from the fp64 value as torch rounds its Python float.
struct SegOpt { float step_size, wd, shrink; bool frozen; };
__device__ __forceinline__ SegOpt seg_opt(const OptArgs& a, int s) {
#pragma clang fp contract(off)
    SegOpt o;
    const float scale = a.nseg > 0 ? a.seg_lr_scale[s] : 1.f;
    const float lr_e = a.lr * scale;
    o.wd = a.nseg > 0 ? a.seg_weight_decay[s] : 0.f;
    o.frozen = a.nseg > 0 && (a.seg_flags[s] & kFrozen);
    o.step_size = lr_e / a.bc1;
    o.shrink = (float)(1.0 - (double)lr_e * (double)o.wd);
    return o;
}

// One element: the gradient scaled by the clip factor, the weight decay in its L2 form (added to the gradient: torch.optim.Adam) or its
// decoupled form (the parameter shrunk first: torch.optim.AdamW), then adam_one.  gs = 1 and wd = 0 leave adam_one's inputs bit-unchanged
// (x * 1 is x; the decay terms are skipped, not added as zeros: -0 + 0 would be +0).
__device__ __forceinline__ void opt_one(float& p, float g, float& m, float& v, float gs, const SegOpt& o, int decoupled, float b1, float b2, float c1,
                                        float c2, float eps, float bc2_sqrt) {
#pragma clang fp contract(off)
    float ge = g * gs;
    if (o.wd != 0.f) {
        if (decoupled) p = p * o.shrink;
        else ge = ge + o.wd * p;
    }
    adam_one(p, ge, m, v, b1, b2, c1, c2, eps, o.step_size, bc2_sqrt);
}

// One thread per four consecutive parameters, as adam_kernel; frozen elements are neither read nor written.
__global__ void __launch_bounds__(TT)
optimizer_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n, OptArgs a) {
    __shared__ int s_first;
    const long long base = (long long)blockIdx.x * TT * 4;
    int s = a.nseg > 0 ? first_segment(a.seg_begin, a.nseg, base, &s_first) : 0;
    const long long i = base + (long long)threadIdx.x * 4;
    if (i >= n) return;
    const float gs = a.record ? (float)a.record[1] : a.grad_scale;
    const float c1 = 1.f - a.b1, c2 = 1.f - a.b2;
    bool whole = i + 4 <= n;
    if (a.nseg > 0) {
        while (a.seg_begin[s + 1] <= i) ++s;         // (i < n = seg_begin[nseg]: s stays below nseg)
        whole = whole && i + 4 <= a.seg_begin[s + 1];
    }
    if (whole) {
        const SegOpt o = seg_opt(a, s);
        if (o.frozen) return;
        float4 pv = *reinterpret_cast<float4*>(p + i), mv = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
        const float4 gv = *reinterpret_cast<const float4*>(g + i);
        opt_one(pv.x, gv.x, mv.x, vv.x, gs, o, a.decoupled, a.b1, a.b2, c1, c2, a.eps, a.bc2_sqrt);
        opt_one(pv.y, gv.y, mv.y, vv.y, gs, o, a.decoupled, a.b1, a.b2, c1, c2, a.eps, a.bc2_sqrt);
        opt_one(pv.z, gv.z, mv.z, vv.z, gs, o, a.decoupled, a.b1, a.b2, c1, c2, a.eps, a.bc2_sqrt);
        opt_one(pv.w, gv.w, mv.w, vv.w, gs, o, a.decoupled, a.b1, a.b2, c1, c2, a.eps, a.bc2_sqrt);
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
        *reinterpret_cast<float4*>(p + i) = pv;
    } else {
        for (long long e = i; e < n && e < i + 4; ++e) {
            if (a.nseg > 0)
                while (a.seg_begin[s + 1] <= e) ++s;
            const SegOpt o = seg_opt(a, s);
            if (o.frozen) continue;
            opt_one(p[e], g[e], m[e], v[e], gs, o, a.decoupled, a.b1, a.b2, c1, c2, a.eps, a.bc2_sqrt);
        }
    }
}

// The table covers [0, n) in strictly increasing order (checked on the caller's host copy: no device-to-host read) and is complete.
int check_segments(const char* who, long long n, int nseg, const void* seg_begin, const long long* seg_begin_host, const void* seg_flags) {
    VIDC_REQUIRE(nseg >= 0, VIDC_ERR_SHAPE, "%s: nseg < 0", who);
    if (nseg == 0) return VIDC_OK;
    VIDC_REQUIRE(seg_begin && seg_begin_host && seg_flags, VIDC_ERR_NULL, "%s: a segment table needs seg_begin, its host copy and seg_flags", who);
    VIDC_REQUIRE(seg_begin_host[0] == 0 && seg_begin_host[nseg] == n, VIDC_ERR_SHAPE, "%s: the segment table covers [%lld, %lld), not [0, %lld)", who,
                 seg_begin_host[0], seg_begin_host[nseg], n);
    for (int s = 0; s < nseg; ++s)
        VIDC_REQUIRE(seg_begin_host[s] < seg_begin_host[s + 1], VIDC_ERR_SHAPE, "%s: seg_begin is not strictly increasing at segment %d", who, s);
    return VIDC_OK;
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

extern "C" size_t vidc_grad_sqnorm_scratch_bytes(long long n) { return n > 0 ? ((size_t)norm_chunks(n) + 8) * sizeof(double) : 0; }

extern "C" int vidc_grad_sqnorm(const float* g, long long n, int nseg, const long long* seg_begin, const long long* seg_begin_host, const int* seg_flags,
                                float grad_scale, float max_norm, double* record, void* scratch, vidc_stream_t stream) {
    VIDC_REQUIRE(g && record && scratch, VIDC_ERR_NULL, "vidc_grad_sqnorm: null pointer");
    VIDC_REQUIRE(n > 0 && n < (1LL << 42), VIDC_ERR_SHAPE, "vidc_grad_sqnorm: bad n");
    VIDC_REQUIRE(aligned16(g) && ((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(record)) & 7) == 0, VIDC_ERR_SHAPE,
                 "vidc_grad_sqnorm: g must be 16-byte aligned, record and scratch 8-byte aligned");
    if (seg_begin == nullptr || seg_flags == nullptr) nseg = 0;
    if (int rc = check_segments("vidc_grad_sqnorm", n, nseg, seg_begin, seg_begin_host, seg_flags)) return rc;
    hipStream_t st = vidc::as_stream(stream);
    const int nb = norm_chunks(n);
    double* partial = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nb), dim3(TT), 0, st, g, n, nseg, seg_begin, seg_flags, partial);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(TT), 0, st, partial, nb, (double)grad_scale, (double)max_norm, record);
    VIDC_CHECK_LAUNCH("grad_sqnorm");
    return VIDC_OK;
}

extern "C" int vidc_grad_accumulate(float* acc, float* g, long long n, int mode, vidc_stream_t stream) {
    VIDC_REQUIRE(acc && g, VIDC_ERR_NULL, "vidc_grad_accumulate: null pointer");
    VIDC_REQUIRE(n > 0 && mode >= 0 && mode <= 2, VIDC_ERR_SHAPE, "vidc_grad_accumulate: bad arguments (mode 0: acc = g, 1: acc += g, 2: g += acc)");
    VIDC_REQUIRE(aligned16(acc, g) && acc != g, VIDC_ERR_SHAPE, "vidc_grad_accumulate: two distinct 16-byte aligned buffers");
    hipStream_t st = vidc::as_stream(stream);
    const dim3 grid(blocks((n + 3) / 4));
    if (mode == 0) hipLaunchKernelGGL(accumulate_kernel<true>, grid, dim3(TT), 0, st, acc, g, n);
    else if (mode == 1) hipLaunchKernelGGL(accumulate_kernel<false>, grid, dim3(TT), 0, st, acc, g, n);
    else hipLaunchKernelGGL(accumulate_kernel<false>, grid, dim3(TT), 0, st, g, acc, n);
    VIDC_CHECK_LAUNCH("accumulate_kernel");
    return VIDC_OK;
}

extern "C" int vidc_optimizer_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
                                   int decoupled, const double* record, float grad_scale, int nseg, const long long* seg_begin,
                                   const long long* seg_begin_host, const float* seg_lr_scale, const float* seg_weight_decay, const int* seg_flags,
                                   vidc_stream_t stream) {
    VIDC_REQUIRE(p && g && m && v, VIDC_ERR_NULL, "vidc_optimizer_step: null pointer");
    VIDC_REQUIRE(n > 0 && step >= 1, VIDC_ERR_SHAPE, "vidc_optimizer_step: bad arguments");
    VIDC_REQUIRE(aligned16(p, g, m, v) && (reinterpret_cast<uintptr_t>(record) & 7) == 0, VIDC_ERR_SHAPE,
                 "vidc_optimizer_step: the four buffers must be 16-byte aligned, record 8-byte aligned");
    if (seg_begin == nullptr || seg_lr_scale == nullptr || seg_weight_decay == nullptr || seg_flags == nullptr) nseg = 0;
    if (int rc = check_segments("vidc_optimizer_step", n, nseg, seg_begin, seg_begin_host, seg_flags)) return rc;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    OptArgs a;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.bc1 = (float)bc1; a.bc2_sqrt = (float)sqrt(bc2); a.grad_scale = grad_scale;
    a.decoupled = decoupled != 0; a.nseg = nseg; a.record = record;
    a.seg_begin = seg_begin; a.seg_lr_scale = seg_lr_scale; a.seg_weight_decay = seg_weight_decay; a.seg_flags = seg_flags;
    hipLaunchKernelGGL(optimizer_kernel, dim3(blocks((n + 3) / 4)), dim3(TT), 0, vidc::as_stream(stream), p, g, m, v, n, a);
    VIDC_CHECK_LAUNCH("optimizer_kernel");
    return VIDC_OK;
}
