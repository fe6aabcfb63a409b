// 2-DoF gravity-aligned homography warp for gfx950 (HBM-bound bilinear gather).
//
// Replaces networks/warping_2dof_alignment.py:35-58,108-156,216-255 of the reference: there the sampling grid is
// materialised through ~520 ATen calls per sample; here a 1-thread-per-sample prologue derives (H, R, H^-1, bbox,
// kw, kh) and one gather kernel maps each output pixel through the homography and samples, so the only HBM traffic
// is the image in and the image out (1.84 MB per 3x240x320 frame).
#include "common.h"

namespace {

// ---- per-sample geometry ---------------------------------------------------------------------------------
__device__ inline void mat3_mul(const float* A, const float* B, float* C) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = A[i * 3 + 0] * B[0 * 3 + j];
            s = s + A[i * 3 + 1] * B[1 * 3 + j];
            s = s + A[i * 3 + 2] * B[2 * 3 + j];
            C[i * 3 + j] = s;
        }
}

__global__ void warp_params_kernel(const float* __restrict__ gravity, const float* __restrict__ aligned, int B, float fx,
                                   float fy, float cx, float cy, const float* __restrict__ Kinv_in, int W, int H,
                                   float* __restrict__ params) {
#pragma clang fp contract(off)
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float g0 = gravity[b * 3 + 0], g1 = gravity[b * 3 + 1], g2 = gravity[b * 3 + 2];
    const float a0 = aligned[b * 3 + 0], a1 = aligned[b * 3 + 1], a2 = aligned[b * 3 + 2];
    // q = (-skew(a)) g = g x a ; rows of -skew(a): [0, a2, -a1], [-a2, 0, a0], [a1, -a0, 0]
    float q0 = a2 * g1 + (-a1) * g2;
    float q1 = (-a2) * g0 + a0 * g2;
    float q2 = a1 * g0 + (-a0) * g1;
    float dot = a0 * g0 + a1 * g1 + a2 * g2;
    float nq = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
    float q4 = cosf(0.5f * atan2f(nq, dot));
    // (the reference's degenerate-rotation branch, :49-50, is dead: its result is overwritten at :53)
    float d = 2.0f * q4;
    q0 = q0 / d; q1 = q1 / d; q2 = q2 / d;
    float S[9] = {0.f, -q2, q1, q2, 0.f, -q0, -q1, q0, 0.f};
    float S2[9], twoS[9];
    for (int i = 0; i < 9; ++i) twoS[i] = 2.0f * S[i];
    mat3_mul(twoS, S, S2);
    float R[9];
    for (int i = 0; i < 9; ++i) {
        float id = (i % 4 == 0) ? 1.0f : 0.0f;
        R[i] = (id + 2.0f * q4 * S[i]) + S2[i];
    }
    float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    float Kinv[9], Rt[9], T[9], Hm[9], Hinv[9];
    for (int i = 0; i < 9; ++i) Kinv[i] = Kinv_in[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = R[j * 3 + i];
    mat3_mul(K, R, T);
    mat3_mul(T, Kinv, Hm);
    mat3_mul(K, Rt, T);
    mat3_mul(T, Kinv, Hinv);
    // bbox of the four projected image corners
    const float cxs[4] = {0.f, (float)(W - 1), 0.f, (float)(W - 1)};
    const float cys[4] = {0.f, 0.f, (float)(H - 1), (float)(H - 1)};
    float px_min = 0.f, px_max = 0.f, py_min = 0.f, py_max = 0.f;
    for (int c = 0; c < 4; ++c) {
        float x = (Hm[0] * cxs[c] + Hm[1] * cys[c]) + Hm[2];
        float y = (Hm[3] * cxs[c] + Hm[4] * cys[c]) + Hm[5];
        float z = (Hm[6] * cxs[c] + Hm[7] * cys[c]) + Hm[8];
        float px = x / z, py = y / z;
        if (c == 0) { px_min = px_max = px; py_min = py_max = py; }
        else {
            px_min = fminf(px_min, px); px_max = fmaxf(px_max, px);
            py_min = fminf(py_min, py); py_max = fmaxf(py_max, py);
        }
    }
    float h_max = py_max - py_min, w_max = px_max - px_min;
    float kw, kh;
    if (w_max > 4.0f * h_max / 3.0f) {
        kw = (float)W / w_max;
        kh = (float)H / (3.0f * w_max / 4.0f);
    } else {
        kh = (float)H / h_max;
        kw = (float)W / (4.0f * h_max / 3.0f);
    }
    float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    for (int i = 0; i < 9; ++i) { p[i] = Hm[i]; p[9 + i] = R[i]; p[18 + i] = Hinv[i]; }
    p[27] = px_min; p[28] = py_min; p[29] = kw; p[30] = kh; p[31] = 0.f;
}

using vidc::Taps;
using vidc::make_taps;
using vidc::sample;
using vidc::warp_fwd_taps;

// Workgroups go to the 8 XCDs (8 private L2s) round-robin in linear launch order; a block of 256 consecutive output pixels gathers from
// source rows that its neighbours need too.  XCD k therefore takes the k-th contiguous band of the (image, pixel block) space instead of
// every eighth block (gridDim.x is a multiple of 8, host side): rocprofv3 FETCH_SIZE was 3.7x the input with the round-robin order.
__device__ __forceinline__ void xcd_band_block(unsigned& bx, unsigned& by) {
    const unsigned gx = gridDim.x, L = blockIdx.y * gx + blockIdx.x, per = (gx >> 3) * gridDim.y;
    const unsigned idx = (L & 7u) * per + (L >> 3);
    by = idx / gx;
    bx = idx - by * gx;
}

// Tap set of output pixel (X, Y) of the inverse warp (warping_2dof_alignment.py:236-247): kw * (H (X, Y, 1) - bbox origin) through make_taps.  The
// adjoint's restatement of warp_inv_rot_norm_kernel's first lines: the same expressions under the same contraction pragma (IEEE operations
// only, so the same bits), kept apart so that the forward kernel's instruction stream stays what it was.
__device__ inline Taps warp_inv_taps(const float* __restrict__ p, int X, int Y, float cx, float cy, int W, int H, int align_corners) {
    const float px_min = p[27], py_min = p[28], kw = p[29], kh = p[30];
    float u, v;
    {
#pragma clang fp contract(off)
        float P0 = (p[0] * (float)X + p[1] * (float)Y) + p[2];
        float P1 = (p[3] * (float)X + p[4] * (float)Y) + p[5];
        float P2 = (p[6] * (float)X + p[7] * (float)Y) + p[8];
        u = kw * (P0 / P2 - px_min);
        v = kh * (P1 / P2 - py_min);
    }
    return make_taps(u, v, cx, cy, W, H, align_corners);
}

// One thread per output pixel (lanes run along X, so the NCHW stores are fully coalesced and the
// gathers of neighbouring lanes hit neighbouring source pixels); all C channels reuse one tap set.
__global__ void __launch_bounds__(256)
warp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ y, int C, int H, int W,
                float cx, float cy, int align_corners) {
    unsigned bx, by;
    xcd_band_block(bx, by);
    const int b = (int)by;
    const int pix = (int)(bx * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int Y = pix / W, X = pix - Y * W;
    const Taps t = warp_fwd_taps(params + (size_t)b * VIDC_WARP_PARAMS, X, Y, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * C * plane;
    float* yb = y + (size_t)b * C * plane + pix;
    for (int c = 0; c < C; ++c) yb[c * plane] = vidc::sample_nt(xb + c * plane, t);      // (x: rewritten by a copy before every launch -- common.h)
}

__global__ void __launch_bounds__(256)
warp_inv_rot_norm_kernel(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ z, int H, int W,
                         float cx, float cy, int align_corners, int normalize) {
    unsigned bx, by;
    xcd_band_block(bx, by);
    const int b = (int)by;
    const int pix = (int)(bx * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int Y = pix / W, X = pix - Y * W;
    const float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    const float px_min = p[27], py_min = p[28], kw = p[29], kh = p[30];
    float u, v;
    {
#pragma clang fp contract(off)
        float P0 = (p[0] * (float)X + p[1] * (float)Y) + p[2];
        float P1 = (p[3] * (float)X + p[4] * (float)Y) + p[5];
        float P2 = (p[6] * (float)X + p[7] * (float)Y) + p[8];
        u = kw * (P0 / P2 - px_min);
        v = kh * (P1 / P2 - py_min);
    }
    Taps t = make_taps(u, v, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * 3 * plane;
    float y0 = vidc::sample_nt(xb, t), y1 = vidc::sample_nt(xb + plane, t), y2 = vidc::sample_nt(xb + 2 * plane, t);      // (x: the head's output of this tick)
    // z = R^T y  (C_R_Cg.bmm(y), warping_2dof_alignment.py:253)
    float z0 = p[9] * y0 + p[12] * y1 + p[15] * y2;
    float z1 = p[10] * y0 + p[13] * y1 + p[16] * y2;
    float z2 = p[11] * y0 + p[14] * y1 + p[17] * y2;
    if (normalize) {   // F.normalize(dim=1): v / max(||v||_2, 1e-12)
        float n = fmaxf(sqrtf(z0 * z0 + z1 * z1 + z2 * z2), 1e-12f);
        z0 /= n; z1 /= n; z2 /= n;
    }
    float* zb = z + (size_t)b * 3 * plane + pix;
    zb[0] = z0; zb[plane] = z1; zb[2 * plane] = z2;
}

// ---- adjoints (dx of the two warps): gather form, bit-reproducible ---------------------------------------------------------------------
// dx[p] = sum over the output pixels q whose tap set contains source pixel p of w(q, p) * dy[q].  A thread owns p.  The taps of q contain p
// only if q's sampling position lies inside the open square (px - 1, px + 1) x (py - 1, py + 1); both sampling maps are a homography composed
// with the bbox shift / scale of the record and the record holds the homography AND its inverse, so the square is mapped into output space in
// closed form.  A homography maps a convex quadrilateral that does not meet its vanishing line (the four denominators share a sign) onto the
// convex hull of the corner images, so the bounding box of those four points holds every candidate q; it is widened by 1/8 pixel + 1/64 of
// its extent for the rounding of the fp32 maps (H and H^-1 are inverse to ~1e-6) and clamped to the image.  A square that meets the vanishing
// line, or a non-finite corner, takes the whole image as its window: any size is walked, none truncated.  Every candidate's taps come from
// the forward's own device functions, so a tap counts exactly when the forward used it; candidates are visited in row-major order and summed
// by one thread: the same bits every run.
struct Window { int x0, x1, y0, y1; };

// the (u, v) coordinate whose sampling position (make_taps) is pixel coordinate i
__device__ inline float pixel_to_uv(float i, float c, int N, int align_corners) {
    const float g = align_corners ? (2.f * i / (float)(N - 1) - 1.f) : ((2.f * i + 1.f) / (float)N - 1.f);
    return g * ((float)N / 2) + c;
}

template <bool INVERSE>
__device__ inline Window adjoint_window(const float* __restrict__ p, int px, int py, float cx, float cy, int W, int H, int align_corners) {
    const float px_min = p[27], py_min = p[28], kw = p[29], kh = p[30];
    float xlo = 0.f, xhi = 0.f, ylo = 0.f, yhi = 0.f, d0 = 0.f;
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
        const float u = pixel_to_uv((float)px + ((k & 1) ? 1.f : -1.f), cx, W, align_corners);
        const float v = pixel_to_uv((float)py + ((k & 2) ? 1.f : -1.f), cy, H, align_corners);
        float qx, qy, d;
        if (INVERSE) {      // u = kw * ((H q)_x - px_min)  =>  q = H^-1 (u / kw + px_min, v / kh + py_min, 1)
            const float s = u / kw + px_min, t = v / kh + py_min;
            d = p[24] * s + p[25] * t + p[26];
            qx = (p[18] * s + p[19] * t + p[20]) / d;
            qy = (p[21] * s + p[22] * t + p[23]) / d;
        } else {            // (u, v) = H^-1 (X / kw + px_min, Y / kh + py_min, 1)  =>  X = kw * ((H (u, v, 1))_x - px_min)
            d = p[6] * u + p[7] * v + p[8];
            qx = kw * ((p[0] * u + p[1] * v + p[2]) / d - px_min);
            qy = kh * ((p[3] * u + p[4] * v + p[5]) / d - py_min);
        }
        if (k == 0) { d0 = d; xlo = xhi = qx; ylo = yhi = qy; }
        ok = ok && (d0 > 0.f ? d > 0.f : d < 0.f) && fabsf(qx) < 1e9f && fabsf(qy) < 1e9f;      // (NaN / inf fail the comparisons)
        xlo = fminf(xlo, qx); xhi = fmaxf(xhi, qx);
        ylo = fminf(ylo, qy); yhi = fmaxf(yhi, qy);
    }
    Window w = {0, W - 1, 0, H - 1};
    if (ok) {
        const float mx = 0.125f + (xhi - xlo) * (1.f / 64), my = 0.125f + (yhi - ylo) * (1.f / 64);
        w.x0 = (int)fminf(fmaxf(floorf(xlo - mx), 0.f), (float)W);          // (an empty window, x0 > x1, where the square maps outside the image)
        w.x1 = (int)fmaxf(fminf(ceilf(xhi + mx), (float)(W - 1)), -1.f);
        w.y0 = (int)fminf(fmaxf(floorf(ylo - my), 0.f), (float)H);
        w.y1 = (int)fmaxf(fminf(ceilf(yhi + my), (float)(H - 1)), -1.f);
    }
    return w;
}

// weight with which tap set t reads plane element o (0 if it does not; a clamped out-of-image tap carries weight 0)
__device__ inline float tap_weight(const Taps& t, int o) {
    return ((t.o00 == o ? t.w00 : 0.f) + (t.o01 == o ? t.w01 : 0.f)) + ((t.o10 == o ? t.w10 : 0.f) + (t.o11 == o ? t.w11 : 0.f));
}

// Adjoint of warp_fwd_kernel.  One thread per SOURCE pixel (lanes along X: coalesced stores; neighbouring threads walk overlapping windows of dy,
// so the blocks are banded over the XCDs like the forward's); four channels share one walk of the window.
__global__ void __launch_bounds__(256)
warp_fwd_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ params, float* __restrict__ dx, int C, int H, int W, float cx,
                    float cy, int align_corners) {
    unsigned bx, by;
    xcd_band_block(bx, by);
    const int b = (int)by;
    const int pix = (int)(bx * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int py = pix / W, px = pix - py * W;
    const float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    const Window win = adjoint_window<false>(p, px, py, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* dyb = dy + (size_t)b * C * plane;
    float* dxb = dx + (size_t)b * C * plane + pix;
    for (int c0 = 0; c0 < C; c0 += 4) {
        const int nc = min(4, C - c0);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int Y = win.y0; Y <= win.y1; ++Y)
            for (int X = win.x0; X <= win.x1; ++X) {
                const Taps t = warp_fwd_taps(p, X, Y, cx, cy, W, H, align_corners);
                const float w = tap_weight(t, pix);
                if (w != 0.f) {
                    const float* g = dyb + (size_t)c0 * plane + (size_t)Y * W + X;
                    for (int k = 0; k < nc; ++k) acc[k] = fmaf(w, g[k * plane], acc[k]);
                }
            }
        for (int k = 0; k < nc; ++k) dxb[(c0 + k) * plane] = acc[k];
    }
}

// Adjoint of warp_inv_rot_norm_kernel through its three stages: F.normalize (dz -> (dz - zh (zh . dz)) / max(|z|, 1e-12), z = R^T y recomputed
// from x with the forward's expressions; dz / 1e-12 below the clamp, as torch differentiates clamp_min), the rotation (dy = R dz) and the
// transposed gather.
__global__ void __launch_bounds__(256)
warp_inv_rot_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dz, const float* __restrict__ params, float* __restrict__ dx,
                             int H, int W, float cx, float cy, int align_corners, int normalize) {
    unsigned bx, by;
    xcd_band_block(bx, by);
    const int b = (int)by;
    const int pix = (int)(bx * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int py = pix / W, px = pix - py * W;
    const float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    const Window win = adjoint_window<true>(p, px, py, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * 3 * plane;
    const float* gb = dz + (size_t)b * 3 * plane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int Y = win.y0; Y <= win.y1; ++Y)
        for (int X = win.x0; X <= win.x1; ++X) {
            const Taps t = warp_inv_taps(p, X, Y, cx, cy, W, H, align_corners);
            const float w = tap_weight(t, pix);
            if (w == 0.f) continue;
            const size_t q = (size_t)Y * W + X;
            float g0 = gb[q], g1 = gb[plane + q], g2 = gb[2 * plane + q];
            if (normalize) {
                const float y0 = sample(xb, t), y1 = sample(xb + plane, t), y2 = sample(xb + 2 * plane, t);
                const float z0 = p[9] * y0 + p[12] * y1 + p[15] * y2;
                const float z1 = p[10] * y0 + p[13] * y1 + p[16] * y2;
                const float z2 = p[11] * y0 + p[14] * y1 + p[17] * y2;
                const float s = sqrtf(z0 * z0 + z1 * z1 + z2 * z2);
                if (s > 1e-12f) {
                    const float h0 = z0 / s, h1 = z1 / s, h2 = z2 / s;
                    const float d = h0 * g0 + h1 * g1 + h2 * g2;
                    g0 = (g0 - h0 * d) / s; g1 = (g1 - h1 * d) / s; g2 = (g2 - h2 * d) / s;
                } else {
                    g0 /= 1e-12f; g1 /= 1e-12f; g2 /= 1e-12f;
                }
            }
            // z_i = sum_j R[j][i] y_j  =>  dy_j = sum_i R[j][i] dz_i
            a0 = fmaf(w, p[9] * g0 + p[10] * g1 + p[11] * g2, a0);
            a1 = fmaf(w, p[12] * g0 + p[13] * g1 + p[14] * g2, a1);
            a2 = fmaf(w, p[15] * g0 + p[16] * g1 + p[17] * g2, a2);
        }
    float* dxb = dx + (size_t)b * 3 * plane + pix;
    dxb[0] = a0; dxb[plane] = a1; dxb[2 * plane] = a2;
}

}  // namespace

extern "C" int vidc_warp2dof_params(const float* gravity, const float* aligned, int B, float fx, float fy, float cx, float cy,
                                    const float* K_inv, int W, int H, float* params, vidc_stream_t stream) {
    VIDC_REQUIRE(gravity && aligned && K_inv && params, VIDC_ERR_NULL, "vidc_warp2dof_params: null pointer");
    VIDC_REQUIRE(B > 0 && W > 1 && H > 1, VIDC_ERR_SHAPE, "vidc_warp2dof_params: bad shape B=%d W=%d H=%d", B, W, H);
    hipLaunchKernelGGL(warp_params_kernel, dim3(vidc::cdiv(B, 64)), dim3(64), 0, vidc::as_stream(stream), gravity, aligned, B,
                       fx, fy, cx, cy, K_inv, W, H, params);
    VIDC_CHECK_LAUNCH("warp_params_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_fwd(const float* x, const float* params, float* y, int B, int C, int H, int W, float cx, float cy,
                                 int align_corners, vidc_stream_t stream) {
    VIDC_REQUIRE(x && params && y, VIDC_ERR_NULL, "vidc_warp2dof_fwd: null pointer");
    VIDC_REQUIRE(B > 0 && C > 0 && H > 1 && W > 1, VIDC_ERR_SHAPE, "vidc_warp2dof_fwd: bad shape");
    hipLaunchKernelGGL(warp_fwd_kernel, dim3((vidc::cdiv(H * W, 256) + 7) / 8 * 8, B), dim3(256), 0, vidc::as_stream(stream), x, params, y, C,
                       H, W, cx, cy, align_corners);
    VIDC_CHECK_LAUNCH("warp_fwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_inv_rot_norm(const float* x, const float* params, float* z, int B, int H, int W, float cx,
                                          float cy, int align_corners, int normalize, vidc_stream_t stream) {
    VIDC_REQUIRE(x && params && z, VIDC_ERR_NULL, "vidc_warp2dof_inv_rot_norm: null pointer");
    VIDC_REQUIRE(B > 0 && H > 1 && W > 1, VIDC_ERR_SHAPE, "vidc_warp2dof_inv_rot_norm: bad shape");
    hipLaunchKernelGGL(warp_inv_rot_norm_kernel, dim3((vidc::cdiv(H * W, 256) + 7) / 8 * 8, B), dim3(256), 0, vidc::as_stream(stream), x,
                       params, z, H, W, cx, cy, align_corners, normalize);
    VIDC_CHECK_LAUNCH("warp_inv_rot_norm_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_fwd_backward(const float* dy, const float* params, float* dx, int B, int C, int H, int W, float cx, float cy,
                                          int align_corners, vidc_stream_t stream) {
    VIDC_REQUIRE(dy && params && dx, VIDC_ERR_NULL, "vidc_warp2dof_fwd_backward: null pointer");
    VIDC_REQUIRE(B > 0 && C > 0 && H > 1 && W > 1 && (long long)H * W < (1ll << 30), VIDC_ERR_SHAPE, "vidc_warp2dof_fwd_backward: bad shape");
    hipLaunchKernelGGL(warp_fwd_bwd_kernel, dim3((vidc::cdiv(H * W, 256) + 7) / 8 * 8, B), dim3(256), 0, vidc::as_stream(stream), dy, params, dx, C,
                       H, W, cx, cy, align_corners);
    VIDC_CHECK_LAUNCH("warp_fwd_bwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_inv_rot_norm_backward(const float* x, const float* dz, const float* params, float* dx, int B, int H, int W, float cx,
                                                   float cy, int align_corners, int normalize, vidc_stream_t stream) {
    VIDC_REQUIRE(x && dz && params && dx, VIDC_ERR_NULL, "vidc_warp2dof_inv_rot_norm_backward: null pointer");
    VIDC_REQUIRE(B > 0 && H > 1 && W > 1 && (long long)H * W < (1ll << 30), VIDC_ERR_SHAPE, "vidc_warp2dof_inv_rot_norm_backward: bad shape");
    hipLaunchKernelGGL(warp_inv_rot_norm_bwd_kernel, dim3((vidc::cdiv(H * W, 256) + 7) / 8 * 8, B), dim3(256), 0, vidc::as_stream(stream), x, dz,
                       params, dx, H, W, cx, cy, align_corners, normalize);
    VIDC_CHECK_LAUNCH("warp_inv_rot_norm_bwd_kernel");
    return VIDC_OK;
}
