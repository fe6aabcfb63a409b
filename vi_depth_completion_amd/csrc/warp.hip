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

// bbox of the four image corners projected by Hm
struct CornerBox { float px_min, px_max, py_min, py_max; };
__device__ inline CornerBox corner_box(const float* __restrict__ Hm, int W, int H) {
#pragma clang fp contract(off)
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
    return {px_min, px_max, py_min, py_max};
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
    const CornerBox box = corner_box(Hm, W, H);
    const float px_min = box.px_min, py_min = box.py_min;
    float h_max = box.py_max - py_min, w_max = box.px_max - px_min;
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
using vidc::sample;
using vidc::warp_fwd_taps;
using vidc::warp_inv_taps;

// Workgroups go to the 8 XCDs (8 private L2s) round-robin in linear launch order; a block of 256 consecutive output pixels gathers from
// source rows that its neighbours need too.  XCD k therefore takes the k-th contiguous band of the (image, pixel block) space instead of
// every eighth block (gridDim.x is a multiple of 8, host side): rocprofv3 FETCH_SIZE was 3.7x the input with the round-robin order.
__device__ __forceinline__ void xcd_band_block(unsigned& bx, unsigned& by) {
    const unsigned gx = gridDim.x, L = blockIdx.y * gx + blockIdx.x, per = (gx >> 3) * gridDim.y;
    const unsigned idx = (L & 7u) * per + (L >> 3);
    by = idx / gx;
    bx = idx - by * gx;
}

// (z0, z1, z2) = R (a0, a1, a2) with R = Cg_R_C, p[9..17] of the record; TRANSPOSE: R^T (a0, a1, a2).  Each row is m0 a0 + m1 a1 + m2 a2 with the
// middle product rounded and the other two fused: what the compiler made of that sum when the bits were pinned by the goldens, written out so that
// it does not depend on which of two products the compiler picks to round.
__device__ inline float rot3_row(float m0, float m1, float m2, float a0, float a1, float a2) { return fmaf(m2, a2, fmaf(m0, a0, m1 * a1)); }
template <bool TRANSPOSE>
__device__ inline void rot3(const float* __restrict__ p, float a0, float a1, float a2, float& z0, float& z1, float& z2) {
    constexpr int si = TRANSPOSE ? 1 : 3, sj = TRANSPOSE ? 3 : 1;
    z0 = rot3_row(p[9], p[9 + sj], p[9 + 2 * sj], a0, a1, a2);
    z1 = rot3_row(p[9 + si], p[9 + si + sj], p[9 + si + 2 * sj], a0, a1, a2);
    z2 = rot3_row(p[9 + 2 * si], p[9 + 2 * si + sj], p[9 + 2 * si + 2 * sj], a0, a1, a2);
}

// One thread per output pixel (lanes run along X, so the NCHW stores are fully coalesced and the
// gathers of neighbouring lanes hit neighbouring source pixels).
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
    const Taps t = warp_inv_taps(p, X, Y, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * 3 * plane;
    float y0 = vidc::sample_nt(xb, t), y1 = vidc::sample_nt(xb + plane, t), y2 = vidc::sample_nt(xb + 2 * plane, t);      // (x: the head's output of this tick)
    float z0, z1, z2;
    rot3<true>(p, y0, y1, y2, z0, z1, z2);      // z = R^T y  (C_R_Cg.bmm(y), warping_2dof_alignment.py:253)
    if (normalize) {   // F.normalize(dim=1): v / max(||v||_2, 1e-12)
        float n = fmaxf(sqrtf(z0 * z0 + z1 * z1 + z2 * z2), 1e-12f);
        z0 /= n; z1 /= n; z2 /= n;
    }
    float* zb = z + (size_t)b * 3 * plane + pix;
    zb[0] = z0; zb[plane] = z1; zb[2 * plane] = z2;
}

// ---- the tap sets of F.grid_sample's three interpolation modes ----------------------------------------------------------------------------
constexpr int kBilinear = VIDC_WARP_BILINEAR, kNearest = VIDC_WARP_NEAREST, kBicubic = VIDC_WARP_BICUBIC;

// the pixel position at which output pixel (X, Y) of the forward warp samples: what warp_fwd_taps floors, with the mode's `far` (common.h)
__device__ inline float2 warp_fwd_pixel(const float* __restrict__ p, int X, int Y, float cx, float cy, int W, int H, int align_corners, float far) {
    return vidc::grid_to_pixel(vidc::warp_grid_xy(vidc::warp_fwd_uv(p, X, Y), cx, cy, W, H), W, H, align_corners, far);
}

// torch's get_cubic_upsample_coefficients (A = -0.75): the weights of taps floor(i) - 1 .. floor(i) + 2 at fraction t
__device__ inline void cubic_weights(float t, float* w) {
#pragma clang fp contract(off)
    constexpr float A = -0.75f;
    const float a = t + 1.f, b = 1.f - t, c = b + 1.f;
    w[0] = ((A * a - 5.f * A) * a + 8.f * A) * a - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * b - (A + 3.f)) * b * b + 1.f;
    w[3] = ((A * c - 5.f * A) * c + 8.f * A) * c - 4.f * A;
}

// weight with which tap set t reads plane element o (0 if it does not; a clamped out-of-image tap carries weight 0)
__device__ inline float tap_weight(const Taps& t, int o) {
    return ((t.o00 == o ? t.w00 : 0.f) + (t.o01 == o ? t.w01 : 0.f)) + ((t.o10 == o ? t.w10 : 0.f) + (t.o11 == o ? t.w11 : 0.f));
}

// One interface per tap set: make() the set of output pixel (X, Y), get() the sample of one H*W plane, weight() the weight with which the set reads
// source pixel (px, py) = plane element pix (0 if it does not; a source pixel is inside the image, so an out-of-image tap never matches).
template <bool INVERSE> struct BilinearTaps {
    Taps t;
    __device__ inline void make(const float* __restrict__ p, int X, int Y, float cx, float cy, int W, int H, int align_corners) {
        t = INVERSE ? warp_inv_taps(p, X, Y, cx, cy, W, H, align_corners) : warp_fwd_taps(p, X, Y, cx, cy, W, H, align_corners);
    }
    __device__ inline float get(const float* __restrict__ plane) const { return vidc::sample_nt(plane, t); }
    __device__ inline float weight(int, int, int pix) const { return tap_weight(t, pix); }
};

template <int MODE> struct ModeTaps;

template <> struct ModeTaps<kBilinear> : BilinearTaps<false> {};

template <> struct ModeTaps<kNearest> {
    int x, y, o;        // the pixel (rint ix, rint iy): ties to even, torch's nearbyint; o: its element offset, clamped into the plane
    bool in;
    __device__ inline void make(const float* __restrict__ p, int X, int Y, float cx, float cy, int W, int H, int align_corners) {
        const float2 pos = warp_fwd_pixel(p, X, Y, cx, cy, W, H, align_corners, -2.0f);
        x = (int)rintf(pos.x); y = (int)rintf(pos.y);
        in = x >= 0 && x < W && y >= 0 && y < H;
        o = min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1);
    }
    __device__ inline float get(const float* __restrict__ plane) const {
        const float v = plane[o];
        return in ? v : 0.f;
    }
    __device__ inline float weight(int px, int py, int) const { return (x == px && y == py) ? 1.f : 0.f; }
};

template <> struct ModeTaps<kBicubic> {
    int x0, y0;                     // floor(ix), floor(iy): tap (i, j) is pixel (x0 - 1 + i, y0 - 1 + j)
    int ox[4], oy[4];               // clamped column / row * W offsets: every load stays inside the plane
    bool vx[4], vy[4];              // ... and whether the tap is inside the image (each of the 16 on its own: zeros padding, no coordinate clamping)
    float wx[4], wy[4];
    __device__ inline void make(const float* __restrict__ p, int X, int Y, float cx, float cy, int W, int H, int align_corners) {
        const float2 pos = warp_fwd_pixel(p, X, Y, cx, cy, W, H, align_corners, -3.0f);
        const float ix = pos.x, iy = pos.y;
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        x0 = (int)fx0; y0 = (int)fy0;
        cubic_weights(ix - fx0, wx);
        cubic_weights(iy - fy0, wy);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = x0 - 1 + i, yy = y0 - 1 + i;
            vx[i] = xx >= 0 && xx < W; vy[i] = yy >= 0 && yy < H;
            ox[i] = min(max(xx, 0), W - 1); oy[i] = min(max(yy, 0), H - 1) * W;
        }
    }
    // rows outer, one fmaf chain per row, then the four row sums: a fixed order, whatever the compiler unrolls
    __device__ inline float get(const float* __restrict__ plane) const {
        float out = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* row = plane + oy[j];
            float r = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = row[ox[i]];
                v = (vx[i] && vy[j]) ? v : 0.f;
                r = (i == 0) ? v * wx[0] : fmaf(v, wx[i], r);
            }
            out = (j == 0) ? r * wy[0] : fmaf(r, wy[j], out);
        }
        return out;
    }
    __device__ inline float weight(int px, int py, int) const {
        const int i = px - x0 + 1, j = py - y0 + 1;
        if (i < 0 || i > 3 || j < 0 || j > 3) return 0.f;
        const float a = i == 0 ? wx[0] : i == 1 ? wx[1] : i == 2 ? wx[2] : wx[3];
        const float b = j == 0 ? wy[0] : j == 1 ? wy[1] : j == 2 ? wy[2] : wy[3];
        return a * b;
    }
};

// The forward warp (warping_2dof_alignment.py:108-156 with interp_mode, :258-290): one thread per output pixel, lanes along X, one tap set for all
// C channels.  ROTATE (C == 3): z = Cg_R_C y in the same store pass (:288), as warp_inv_rot_norm_kernel does with R^T.
template <int MODE, bool ROTATE>
__global__ void __launch_bounds__(256)
warp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ y, int C, int H, int W,
                float cx, float cy, int align_corners) {
    unsigned bx, by;
    xcd_band_block(bx, by);
    const int b = (int)by;
    const int pix = (int)(bx * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int Y = pix / W, X = pix - Y * W;
    const float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    ModeTaps<MODE> t;
    t.make(p, X, Y, cx, cy, W, H, align_corners);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * C * plane;
    float* yb = y + (size_t)b * C * plane + pix;
    if (ROTATE) {
        const float y0 = t.get(xb), y1 = t.get(xb + plane), y2 = t.get(xb + 2 * plane);
        float z0, z1, z2;
        rot3<false>(p, y0, y1, y2, z0, z1, z2);
        yb[0] = z0; yb[plane] = z1; yb[2 * plane] = z2;
    } else {
        for (int c = 0; c < C; ++c) yb[c * plane] = t.get(xb + c * plane);      // (x: rewritten by a copy before every launch -- common.h)
    }
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

// hw: the half-width of the interpolation's support in pixels -- 1 for bilinear and nearest (the square above), 2 for bicubic, whose taps reach from
// floor(ix) - 1 to floor(ix) + 2.
template <bool INVERSE>
__device__ inline Window adjoint_window(const float* __restrict__ p, int px, int py, float cx, float cy, int W, int H, int align_corners, float hw) {
    const float px_min = p[27], py_min = p[28], kw = p[29], kh = p[30];
    float xlo = 0.f, xhi = 0.f, ylo = 0.f, yhi = 0.f, d0 = 0.f;
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
        const float u = pixel_to_uv((float)px + ((k & 1) ? hw : -hw), cx, W, align_corners);
        const float v = pixel_to_uv((float)py + ((k & 2) ? hw : -hw), cy, H, align_corners);
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

// Adjoint of warp_fwd_kernel, its exact transpose.  One thread per SOURCE pixel (lanes along X: coalesced stores; neighbouring threads walk overlapping
// windows of dy, so the blocks are banded over the XCDs like the forward's); the window has the mode's support half-width (1, or 2 for bicubic) and
// the weights are the forward's own; four channels share one walk.  ROTATE (C == 3): dy is first multiplied by Cg_R_C^T (z_i = sum_j R[i][j] y_j  =>
// dy_j = sum_i R[i][j] dz_i).
template <int MODE, bool ROTATE>
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
    const Window win = adjoint_window<false>(p, px, py, cx, cy, W, H, align_corners, MODE == kBicubic ? 2.f : 1.f);
    const size_t plane = (size_t)H * W;
    const float* dyb = dy + (size_t)b * C * plane;
    float* dxb = dx + (size_t)b * C * plane + pix;
    for (int c0 = 0; c0 < C; c0 += 4) {
        const int nc = min(4, C - c0);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int Y = win.y0; Y <= win.y1; ++Y)
            for (int X = win.x0; X <= win.x1; ++X) {
                ModeTaps<MODE> t;
                t.make(p, X, Y, cx, cy, W, H, align_corners);
                const float w = t.weight(px, py, pix);
                if (w != 0.f) {
                    const float* g = dyb + (size_t)c0 * plane + (size_t)Y * W + X;
                    if (ROTATE) {
                        float g0, g1, g2;
                        rot3<true>(p, g[0], g[plane], g[2 * plane], g0, g1, g2);
                        acc[0] = fmaf(w, g0, acc[0]);
                        acc[1] = fmaf(w, g1, acc[1]);
                        acc[2] = fmaf(w, g2, acc[2]);
                    } else {
                        for (int k = 0; k < nc; ++k) acc[k] = fmaf(w, g[k * plane], acc[k]);
                    }
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
    const Window win = adjoint_window<true>(p, px, py, cx, cy, W, H, align_corners, 1.f);
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
                float z0, z1, z2;
                rot3<true>(p, y0, y1, y2, z0, z1, z2);
                const float s = sqrtf(z0 * z0 + z1 * z1 + z2 * z2);
                if (s > 1e-12f) {
                    const float h0 = z0 / s, h1 = z1 / s, h2 = z2 / s;
                    const float d = h0 * g0 + h1 * g1 + h2 * g2;
                    g0 = (g0 - h0 * d) / s; g1 = (g1 - h1 * d) / s; g2 = (g2 - h2 * d) / s;
                } else {
                    g0 /= 1e-12f; g1 /= 1e-12f; g2 /= 1e-12f;
                }
            }
            float d0, d1, d2;
            rot3<false>(p, g0, g1, g2, d0, d1, d2);      // z_i = sum_j R[j][i] y_j  =>  dy_j = sum_i R[j][i] dz_i
            a0 = fmaf(w, d0, a0);
            a1 = fmaf(w, d1, a1);
            a2 = fmaf(w, d2, a2);
        }
    float* dxb = dx + (size_t)b * 3 * plane + pix;
    dxb[0] = a0; dxb[plane] = a1; dxb[2 * plane] = a2;
}

// ---- the sampler grids ---------------------------------------------------------------------------------------------------------------------
// image_sampler_forward_inverse's "give up" rule (warping_2dof_alignment.py:168-179): w_max / h_max of the projected corner box outside [0.8, 2.2],
// from the record's Cg_H_C (the record keeps its 32 words; NaN compares false, as in the reference).
__device__ inline bool warp_gives_up(const float* __restrict__ Hm, int W, int H) {
#pragma clang fp contract(off)
    const CornerBox box = corner_box(Hm, W, H);
    const float scale_sigma = (box.px_max - box.px_min) / (box.py_max - box.py_min);
    return scale_sigma < 0.8f || scale_sigma > 2.2f;
}

// One thread per pixel writes the (gx, gy) pair of both grids; the first thread of a sample writes its 3x3 matrix.  (No gather here: the blocks
// keep their launch order.)  This kernel RESTATES warp_fwd_uv, warp_inv_uv and warp_grid_xy (common.h) in one block instead of calling them: composed
// from the three it has the same instructions in another order and measured 22.7 - 22.8 us against 22.3 - 22.4 us at B = 32 (profiles/EXPERIMENTS.md),
// so this one fold was taken back.  tests/test_warp_modes.py holds the restatement to the gather kernels' bits (nearest against F.grid_sample through
// these grids, bit for bit).
__global__ void __launch_bounds__(256)
warp_grids_kernel(const float* __restrict__ params, float2* __restrict__ grid, float2* __restrict__ inv_grid, float* __restrict__ c_r_cg, int H,
                  int W, float cx, float cy) {
    const int b = (int)blockIdx.y;
    const int pix = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int Y = pix / W, X = pix - Y * W;
    const float* p = params + (size_t)b * VIDC_WARP_PARAMS;
    const bool identity = warp_gives_up(p, W, H);
    float fu, fv, iu, iv;
    if (identity) {
        fu = iu = (float)X;
        fv = iv = (float)Y;
    } else {
        const float px_min = p[27], py_min = p[28], kw = p[29], kh = p[30];
        float F0, F1, F2, I0, I1, I2;
        {
#pragma clang fp contract(off)
            const float Xs = (1.0f / kw) * (float)X + px_min;
            const float Ys = (1.0f / kh) * (float)Y + py_min;
            F0 = (p[18] * Xs + p[19] * Ys) + p[20];
            F1 = (p[21] * Xs + p[22] * Ys) + p[23];
            F2 = (p[24] * Xs + p[25] * Ys) + p[26];
            I0 = (p[0] * (float)X + p[1] * (float)Y) + p[2];
            I1 = (p[3] * (float)X + p[4] * (float)Y) + p[5];
            I2 = (p[6] * (float)X + p[7] * (float)Y) + p[8];
            iu = kw * (I0 / I2 - px_min);
            iv = kh * (I1 / I2 - py_min);
        }
        fu = F0 / F2;
        fv = F1 / F2;
    }
    const float sx = 1.0f / ((float)W / 2), sy = 1.0f / ((float)H / 2);
    const size_t q = (size_t)b * H * W + pix;
    grid[q] = make_float2(sx * (fu - cx), sy * (fv - cy));
    inv_grid[q] = make_float2(sx * (iu - cx), sy * (iv - cy));
    if (pix == 0)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) c_r_cg[b * 9 + i * 3 + j] = identity ? (i == j ? 1.f : 0.f) : p[9 + j * 3 + i];
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
// what every entry that takes an image refuses: the kernels index pixels with int
int check_image(const char* who, bool pointers, int B, int C, int H, int W) {
    VIDC_REQUIRE(pointers, VIDC_ERR_NULL, "%s: null pointer", who);
    VIDC_REQUIRE(B > 0 && C > 0 && H > 1 && W > 1 && (long long)H * W < (1ll << 30), VIDC_ERR_SHAPE, "%s: bad shape", who);
    return VIDC_OK;
}

// one block per 256 pixels, rounded up to whole rounds of the 8 XCDs (xcd_band_block)
dim3 banded_grid(int B, int H, int W) { return dim3((vidc::cdiv(H * W, 256) + 7) / 8 * 8, B); }

template <int MODE, bool ROTATE>
int launch_warp(bool backward, const float* in, const float* params, float* out, int B, int C, int H, int W, float cx, float cy,
                int align_corners, vidc_stream_t stream) {
    if (backward) {
        hipLaunchKernelGGL((warp_fwd_bwd_kernel<MODE, ROTATE>), banded_grid(B, H, W), dim3(256), 0, vidc::as_stream(stream), in, params, out, C, H, W,
                           cx, cy, align_corners);
        VIDC_CHECK_LAUNCH("warp_fwd_bwd_kernel");
    } else {
        hipLaunchKernelGGL((warp_fwd_kernel<MODE, ROTATE>), banded_grid(B, H, W), dim3(256), 0, vidc::as_stream(stream), in, params, out, C, H, W, cx,
                           cy, align_corners);
        VIDC_CHECK_LAUNCH("warp_fwd_kernel");
    }
    return VIDC_OK;
}

// vidc_warp2dof_fwd_mode and its adjoint: their refusals, then the instantiation of (mode, rotate)
int warp_mode_entry(const char* who, bool backward, const float* in, const float* params, float* out, int B, int C, int H, int W, float cx, float cy,
                    int align_corners, int mode, int rotate, vidc_stream_t stream) {
    if (int e = check_image(who, in && params && out, B, C, H, W)) return e;
    VIDC_REQUIRE(mode >= VIDC_WARP_BILINEAR && mode <= VIDC_WARP_BICUBIC, VIDC_ERR_SHAPE, "%s: mode %d is none of 0 (bilinear), 1 (nearest), 2 (bicubic)", who, mode);
    VIDC_REQUIRE(!rotate || C == 3, VIDC_ERR_SHAPE, "%s: rotate needs C == 3 (got %d)", who, C);
    switch (mode * 2 + (rotate ? 1 : 0)) {
        case 0: return launch_warp<kBilinear, false>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
        case 1: return launch_warp<kBilinear, true>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
        case 2: return launch_warp<kNearest, false>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
        case 3: return launch_warp<kNearest, true>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
        case 4: return launch_warp<kBicubic, false>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
        default: return launch_warp<kBicubic, true>(backward, in, params, out, B, C, H, W, cx, cy, align_corners, stream);
    }
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
    if (int e = check_image("vidc_warp2dof_fwd", x && params && y, B, C, H, W)) return e;
    return launch_warp<kBilinear, false>(false, x, params, y, B, C, H, W, cx, cy, align_corners, stream);
}

extern "C" int vidc_warp2dof_fwd_backward(const float* dy, const float* params, float* dx, int B, int C, int H, int W, float cx, float cy,
                                          int align_corners, vidc_stream_t stream) {
    if (int e = check_image("vidc_warp2dof_fwd_backward", dy && params && dx, B, C, H, W)) return e;
    return launch_warp<kBilinear, false>(true, dy, params, dx, B, C, H, W, cx, cy, align_corners, stream);
}

extern "C" int vidc_warp2dof_inv_rot_norm(const float* x, const float* params, float* z, int B, int H, int W, float cx,
                                          float cy, int align_corners, int normalize, vidc_stream_t stream) {
    if (int e = check_image("vidc_warp2dof_inv_rot_norm", x && params && z, B, 3, H, W)) return e;
    hipLaunchKernelGGL(warp_inv_rot_norm_kernel, banded_grid(B, H, W), dim3(256), 0, vidc::as_stream(stream), x, params, z, H, W, cx, cy,
                       align_corners, normalize);
    VIDC_CHECK_LAUNCH("warp_inv_rot_norm_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_inv_rot_norm_backward(const float* x, const float* dz, const float* params, float* dx, int B, int H, int W, float cx,
                                                   float cy, int align_corners, int normalize, vidc_stream_t stream) {
    if (int e = check_image("vidc_warp2dof_inv_rot_norm_backward", x && dz && params && dx, B, 3, H, W)) return e;
    hipLaunchKernelGGL(warp_inv_rot_norm_bwd_kernel, banded_grid(B, H, W), dim3(256), 0, vidc::as_stream(stream), x, dz, params, dx, H, W, cx, cy,
                       align_corners, normalize);
    VIDC_CHECK_LAUNCH("warp_inv_rot_norm_bwd_kernel");
    return VIDC_OK;
}

extern "C" int vidc_warp2dof_fwd_mode(const float* x, const float* params, float* y, int B, int C, int H, int W, float cx, float cy,
                                      int align_corners, int mode, int rotate, vidc_stream_t stream) {
    return warp_mode_entry("vidc_warp2dof_fwd_mode", false, x, params, y, B, C, H, W, cx, cy, align_corners, mode, rotate, stream);
}

extern "C" int vidc_warp2dof_fwd_mode_backward(const float* dy, const float* params, float* dx, int B, int C, int H, int W, float cx, float cy,
                                               int align_corners, int mode, int rotate, vidc_stream_t stream) {
    return warp_mode_entry("vidc_warp2dof_fwd_mode_backward", true, dy, params, dx, B, C, H, W, cx, cy, align_corners, mode, rotate, stream);
}

extern "C" int vidc_warp2dof_grids(const float* params, float* grid, float* inv_grid, float* c_r_cg, int B, int H, int W, float cx, float cy,
                                   vidc_stream_t stream) {
    if (int e = check_image("vidc_warp2dof_grids", params && grid && inv_grid && c_r_cg, B, 1, H, W)) return e;
    VIDC_REQUIRE(((uintptr_t)grid | (uintptr_t)inv_grid) % 8 == 0, VIDC_ERR_SHAPE, "vidc_warp2dof_grids: the grids are stored as (gx, gy) pairs, 8-byte aligned");
    hipLaunchKernelGGL(warp_grids_kernel, dim3(vidc::cdiv(H * W, 256), B), dim3(256), 0, vidc::as_stream(stream), params,
                       reinterpret_cast<float2*>(grid), reinterpret_cast<float2*>(inv_grid), c_r_cg, H, W, cx, cy);
    VIDC_CHECK_LAUNCH("warp_grids_kernel");
    return VIDC_OK;
}
