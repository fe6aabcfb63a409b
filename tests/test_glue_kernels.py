"""The forward glue kernels (csrc/pointwise.hip), entry by entry through the C ABI, at the smallest shapes that reach each of their branches.

tests/test_hip_parity.py reaches the stem conv, the max-pool, the bilinear upsample and the prediction head through the ops.* wrappers on
contiguous tensors (ldx == ldy == C, the split image exactly as wide as the tensor) at flat tolerances.  Here every entry is called with
buffers the test owns: fp32 outputs pre-filled with NaN, -7777.0 in the ld - C gap columns of every row, 0xFF bytes in the split images,
a guard region behind every output, all compared for equality after the call; B = 2 with different data per image (the upsample's grid-row
cases B * H = 1, 31 and 33 cannot have two images and run with B = 1); ldy > C, ldx > G * C, a split slice at split_ch0 > 0.

References are float64 and read only the kernel's fp32 inputs.  Bounds are elementwise, built from the reference's own magnitudes
(u = 2^-24, the unit roundoff of fp32), never from the kernel's output or a fraction of a tensor's maximum.  Counted roundings behind each
factor (reading the kernels; measured ratios: profiles/EXPERIMENTS.md, "glue and metrics kernels one by one"):

  stem      (9 Cin + 2) u conv(|x|, |w|)     one chain acc += patch * w over 9 Cin taps: 9 Cin products and 9 Cin sums, every term passes
                                             through at most 9 Cin + 1 roundings (fewer where hipcc fuses a product and its sum); the ReLU is
                                             1-Lipschitz and rounds nothing.
  max-pool  equality                         fmaxf rounds nothing.
  upsample  8u S |w_i v_i|                   a term hy * hx * v: hx = fl(1 - lx), hx * v, the inner sum, hy = fl(1 - ly), hy * (.), the outer
            + 2u s_y max|d_y| + 2u s_x max|d_x|    sum: 6 roundings, 8u with the second-order terms to spare.  The source coordinate
                                             s = fl(scale * dst) carries one rounding (|s - scale * dst| <= u s; i0 = (int)s and l = s - i0 are
                                             exact), and the interpolant is piecewise linear and continuous in s, so the value moves by at most
                                             |s - s_ref| times the slope |d| of a segment next to the sample point: the one that holds it and
                                             its neighbour on the nearer side (near an integer s the kernel may sit on either).  The reference
                                             takes scale = fl((in - 1) / (out - 1)) in fp32 like ATen and the kernel, and scale * dst in
                                             float64; the second u s allows the division half an ulp more than correct rounding gives it.
            + u (|a| + |b|) per sum a + b    VIDC_UP_ACCUM and the group sum add one rounding per addition (the first, onto 0, is exact).
            EXACT cases: equality            (in - 1) / (out - 1) dyadic, data on a 2^-8 grid: every product and sum is exact.
  head      (ceil(Cin / 64) + 8) u (S |x w| + |bias|)    a lane's chain over ceil(Cin / 64) channels (product and sum each), six levels of
                                             the shuffle tree, the bias: ceil(Cin / 64) + 1 + 6 + 1 roundings at most on any term.
            y: the upsample bound            against the float64 upsample of the `lowres` buffer the device wrote (the second kernel's input).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_NULL, ERR_SHAPE = -1, -2                                       # include/vidc.h
UP_RELU, UP_ACCUM, UP_NO_F32_OUT = 1, 2, 4                         # vidc_up_flags
U = 2.0 ** -24
F32 = np.float32
SENTINEL, GUARD, HUGE = -7777.0, 64, 1.0e9                         # HUGE: what the ldx - C gap of every INPUT row holds
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _L():
    from vi_depth_completion_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Out:
    """A device output pre-filled with `fill`, GUARD untouchable elements behind it."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[:n].view(*shape)
        self.guard = self.whole[n:].clone()

    def ptr(self, offset=0):
        return self.t.data_ptr() + offset * self.t.element_size()

    def np(self):
        assert torch.equal(self.whole[self.t.numel():].view(torch.uint8), self.guard.view(torch.uint8)), "the guard region was written"
        return self.t.cpu().numpy()


class _Rows(_Out):
    """An fp32 output [rows][ld] whose channels c0 .. c0 + C hold NaN (or `base`) and every other column SENTINEL."""

    def __init__(self, rows, C, ld, c0=0, base=None):
        super().__init__((rows, ld), torch.float32, SENTINEL)
        self.c0, self.C = c0, C
        self.t[:, c0:c0 + C] = float("nan") if base is None else _dev(base)

    def values(self):
        a = self.np()
        gap = np.delete(a, np.s_[self.c0:self.c0 + self.C], axis=1)
        assert (gap == F32(SENTINEL)).all(), "a gap column was written"
        return a[:, self.c0:self.c0 + self.C]

    def untouched(self):
        v = self.values()
        return np.isnan(v).all()


def _split_out(rows, ld):
    return _Out((rows, ld * 2), torch.int16, -1)                   # 0xFF bytes


def _split_ref(vals, ld, c0=0):
    """The split image of an [rows][ld] tensor whose channels c0 .. c0 + C hold `vals` (fp32): per row and unit of 32 channels, 32 hi halves
    then 32 lo halves, hi = bf16 RNE of x, lo = bf16 RNE of x - hi (tests/bf16_ref.py); 0xFFFF wherever nothing was stored."""
    x = torch.from_numpy(np.ascontiguousarray(vals, F32))
    hi = bf16_ref.bits(x)
    lo = bf16_ref.bits(x - bf16_ref.rounded(x))
    rows, C = vals.shape
    img = np.full((rows, ld // 32, 2, 32), 0xFFFF, np.uint16)
    c = np.arange(c0, c0 + C)
    img[:, c // 32, 0, c % 32] = hi.numpy().astype(np.uint16)
    img[:, c // 32, 1, c % 32] = lo.numpy().astype(np.uint16)
    return img.reshape(rows, ld * 2)


def _image(out):
    return out.np().view(np.uint16)


WORST = {}


def _hold(name, got, want, bound):
    """|got - want| <= bound elementwise; prints and records the largest error / bound."""
    err = np.abs(got.astype(np.float64) - want)
    assert not np.isnan(got).any(), "%s: an element was not written" % name
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    kernel = name.split()[0]
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print("%s: error / bound %.3f (largest of %s so far %.3f)" % (name, ratio, kernel, WORST[kernel]))
    assert (err <= bound).all(), (name, ratio, np.argwhere(err > bound)[:4])


def _wide(C):
    return (C + 32) // 32 * 32 + 32                                # the next multiple of 32 above C + 32


# ======================================================================================================================================
# stem
# ======================================================================================================================================
# H, W, Cin, Cout, relu, ldy
STEM = [(3, 3, 1, 1, 0, 1), (3, 3, 3, 64, 1, 128), (4, 6, 3, 32, 1, 32), (4, 6, 1, 100, 0, 100), (5, 127, 3, 64, 0, 64), (5, 127, 1, 32, 1, 96),
        (5, 129, 3, 100, 1, 160), (5, 129, 3, 100, 0, 160), (5, 129, 1, 1, 1, 64), (7, 258, 3, 64, 1, 64), (7, 258, 1, 100, 1, 100)]


@functools.lru_cache(maxsize=None)
def _stem_case(H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * 100000 + W * 100 + Cin * 7 + Cout)
    x = torch.randn(2, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.3
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, 2, 1)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout).numpy()      # noqa: E731
    return x, w, rows(ref), rows(mag)


def _stem(x, w, relu, y_ptr, ldy, ysp=None, ch0=0):
    L = _L()
    B, Cin, H, W = x.shape
    L.check(L.lib().vidc_stem_conv3x3s2(L.ptr(x), L.ptr(w), y_ptr, B, Cin, H, W, w.shape[0], ldy, relu, ysp, ch0, L.current_stream()), "stem")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("H,W,Cin,Cout,relu,ldy", STEM, ids=["%dx%d_cin%d_cout%d_relu%d_ld%d" % c for c in STEM])
def test_stem(H, W, Cin, Cout, relu, ldy):
    x, w, ref, mag = _stem_case(H, W, Cin, Cout)
    y = _Rows(ref.shape[0], Cout, ldy)
    _stem(x.to(DEV), w.to(DEV), relu, y.ptr(), ldy)
    want = np.maximum(ref, 0.0) if relu else ref
    if not relu:
        assert (want < 0).any()
    _hold("stem %dx%d cin %d cout %d" % (H, W, Cin, Cout), y.values(), want, (9 * Cin + 2) * U * mag)


@gpu
def test_stem_split_slice():
    """Cout = 32 written as the channels 32..63 of a 96-wide tensor: the fp32 slice, and the slice of the tensor's split image (0xFF
    everywhere else); then the image alone (y == NULL), the same bits."""
    H, W, Cin, Cout, ld, ch0 = 5, 129, 3, 32, 96, 32
    x, w, ref, mag = _stem_case(H, W, Cin, Cout)
    y, img = _Rows(ref.shape[0], Cout, ld, ch0), _split_out(ref.shape[0], ld)
    _stem(x.to(DEV), w.to(DEV), 1, y.ptr(ch0), ld, img.ptr(), ch0)
    got = y.values()
    _hold("stem split slice", got, np.maximum(ref, 0.0), (9 * Cin + 2) * U * mag)
    want = _split_ref(got, ld, ch0)
    assert np.array_equal(_image(img), want)
    alone = _split_out(ref.shape[0], ld)
    _stem(x.to(DEV), w.to(DEV), 1, None, ld, alone.ptr(), ch0)
    assert np.array_equal(_image(alone), want)


@gpu
@pytest.mark.parametrize("align_corners", [0, 1])
def test_stem_through_the_warp_is_the_stem_of_the_stored_warp(align_corners):
    """(37, 53), intrinsics scaled to that image, a near-upright gravity and one of the extreme tilts (tests/golden/warp_cases.npz):
    vidc_stem_conv3x3s2_warped == vidc_stem_conv3x3s2 of what vidc_warp2dof_fwd stored, bit for bit, fp32 slice and split image.
    Forward only."""
    from vi_depth_completion_amd.networks.warping_2dof_alignment import Warping2DOFAlignment
    L = _L()
    lib, st = L.lib(), L.current_stream()
    H, W, Cout, ld, ch0 = 37, 53, 64, 96, 32
    cases = np.load(os.path.join(GOLDEN, "warp_cases.npz"))
    sx, sy = W / 320.0, H / 240.0
    wp = Warping2DOFAlignment(float(cases["fx"]) * sx, float(cases["fy"]) * sy, float(cases["cx"]) * sx, float(cases["cy"]) * sy, bool(align_corners))
    assert (wp.H, wp.W) == (H, W)
    pick = [2, 9]
    assert cases["gravity"][2, 1] > 0.9999 and cases["gravity"][9, 1] < 0.5
    g, a = _dev(cases["gravity"][pick]), _dev(cases["aligned"][pick])
    gen = torch.Generator().manual_seed(37053)
    x = torch.rand(2, 3, H, W, generator=gen).to(DEV)
    w = (torch.randn(Cout, 3, 3, 3, generator=gen) * 0.2).to(DEV)
    params = wp._params(g, a)
    warped = _Out((2, 3, H, W), torch.float32, float("nan"))
    L.check(lib.vidc_warp2dof_fwd(L.ptr(x), L.ptr(params), warped.ptr(), 2, 3, H, W, wp.cx, wp.cy, align_corners, st), "warp")
    rows = 2 * 19 * 27
    y0, i0, y1, i1 = _Rows(rows, Cout, ld, ch0), _split_out(rows, ld), _Rows(rows, Cout, ld, ch0), _split_out(rows, ld)
    _stem(warped.t, w, 1, y0.ptr(ch0), ld, i0.ptr(), ch0)
    L.check(lib.vidc_stem_conv3x3s2_warped(L.ptr(x), L.ptr(params), L.ptr(w), y1.ptr(ch0), 2, H, W, Cout, ld, 1, i1.ptr(), ch0, wp.cx, wp.cy,
                                           align_corners, st), "warped stem")
    torch.cuda.synchronize()
    stored = warped.np()
    assert not np.isnan(stored).any() and (stored[0] != stored[1]).any()
    a0, a1 = y0.values(), y1.values()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and a0.max() > 0.1 and not np.isnan(a0).any()
    assert np.array_equal(_image(i0), _image(i1)) and np.array_equal(_image(i1), _split_ref(a1, ld, ch0))


# ======================================================================================================================================
# max-pool
# ======================================================================================================================================
# H, W, C, ldx, ldy
POOL = [(1, 1, 4, 4, 4), (2, 2, 4, 8, 12), (1, 9, 8, 8, 32), (7, 9, 132, 136, 160), (6, 65, 280, 280, 288)]


@functools.lru_cache(maxsize=None)
def _pool_case(H, W, C, ldx, inf=True):
    """x [2][H][W][ldx] (HUGE in the gap columns), a fifth of the values -inf, the window of output (0, 0) of image 0 all -inf."""
    g = torch.Generator().manual_seed(H * 10000 + W * 100 + C)
    x = torch.randn(2, H, W, ldx, generator=g)
    if inf:
        x[torch.rand(2, H, W, ldx, generator=g) < 0.2] = float("-inf")
        x[0, :2, :2] = float("-inf")
    x[..., C:] = HUGE
    ref = F.max_pool2d(x[..., :C].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    return x, ref.reshape(-1, C).numpy()


def _pool(x, C, y_ptr, ldy, ysp=None):
    L = _L()
    B, H, W, ldx = x.shape
    L.check(L.lib().vidc_maxpool3x3s2(L.ptr(x), y_ptr, B, H, W, C, ldx, ldy, ysp, L.current_stream()), "maxpool")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("H,W,C,ldx,ldy", POOL, ids=["%dx%d_c%d_ldx%d_ldy%d" % c for c in POOL])
def test_maxpool(H, W, C, ldx, ldy):
    x, ref = _pool_case(H, W, C, ldx)
    assert np.isneginf(ref[0]).all() and not np.isneginf(ref).all() and not np.isnan(ref).any()
    y = _Rows(ref.shape[0], C, ldy)
    _pool(x.to(DEV), C, y.ptr(), ldy)
    got = y.values()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]


@gpu
def test_maxpool_split_image():
    H, W, C, ldx, ldy = 7, 9, 132, 136, 160
    x, ref = _pool_case(H, W, C, ldx, inf=False)
    y, img = _Rows(ref.shape[0], C, ldy), _split_out(ref.shape[0], ldy)
    _pool(x.to(DEV), C, y.ptr(), ldy, img.ptr())
    assert np.array_equal(y.values(), ref)
    want = _split_ref(ref, ldy)
    assert np.array_equal(_image(img), want)
    alone = _split_out(ref.shape[0], ldy)
    _pool(x.to(DEV), C, None, ldy, alone.ptr())
    assert np.array_equal(_image(alone), want)


# ======================================================================================================================================
# bilinear upsample, align_corners = True
# ======================================================================================================================================
def _axis(n_in, n_out):
    """The kernel's src_index with scale in fp32 (ATen's value) and scale * dst in float64 -> i0, i1, l, s, and per output index the (up to)
    two segments [k, k + 1] next to the sample point: the one that holds it and its neighbour on the nearer side (-1: none)."""
    scale = float(F32(n_in - 1) / F32(n_out - 1)) if n_out > 1 else 0.0
    s = scale * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l = s - i0
    near = np.where(l < 0.5, i0 - 1, i0 + 1)
    seg = np.stack([i0, near], 1)
    seg[(seg < 0) | (seg > n_in - 2)] = -1
    return i0, i1, l, s, seg


def _seg_max(d, seg, axis):
    """max over the segments seg [n_out][2] of d (segments along `axis`), 0 where a segment is -1."""
    if d.shape[axis] == 0:
        shape = list(d.shape)
        shape[axis] = seg.shape[0]
        return np.zeros(shape)
    out = 0.0
    for j in range(2):
        t = np.take(d, np.maximum(seg[:, j], 0), axis=axis)
        mask = (seg[:, j] >= 0).reshape([-1 if a == axis else 1 for a in range(d.ndim)])
        out = np.maximum(out, t * mask)
    return out


def _up_ref(x, H, W):
    """x float64 [B][h][w][C] -> the float64 interpolation [B][H][W][C], S |w_i v_i|, and the two coordinate terms s max|d| (y, x)."""
    h, w = x.shape[1:3]
    y0, y1, ly, sy, segy = _axis(h, H)
    x0, x1, lx, sx, segx = _axis(w, W)
    ly_, lx_ = ly[None, :, None, None], lx[None, None, :, None]
    cols = lambda t: (1 - lx_) * t[:, :, x0] + lx_ * t[:, :, x1]      # noqa: E731      [B][.][W][C]
    rowsi = lambda t: (1 - ly_) * t[:, y0] + ly_ * t[:, y1]           # noqa: E731      [B][H][.][C]
    val = rowsi(cols(x))
    mag = rowsi(cols(np.abs(x)))
    dy = _seg_max(np.abs(np.diff(cols(x), axis=1)), segy, 1) * sy[None, :, None, None]
    dx = _seg_max(np.abs(np.diff(rowsi(x), axis=2)), segx, 2) * sx[None, None, :, None]
    return val, mag, dy, dx


def _up_expect(x, base, H, W, C, G, flags):
    """x fp32 [B][h][w][ldx] with G groups of C channels, base fp32 [B*H*W][C] or None -> the value and its bound, [B*H*W][C]."""
    total = None if base is None else base.astype(np.float64)
    tmag = None if base is None else np.abs(total)
    bound = 0.0
    for g in range(G):
        val, mag, dy, dx = _up_ref(x[..., g * C:(g + 1) * C].astype(np.float64), H, W)
        if flags & UP_RELU:
            val = np.maximum(val, 0.0)
        val, b = val.reshape(-1, C), (8 * U * mag + 2 * U * dy + 2 * U * dx).reshape(-1, C)
        bound = bound + b
        if total is None:
            total, tmag = val, np.abs(val)
        else:
            total, tmag = total + val, tmag + np.abs(val)
            bound = bound + U * tmag                               # one rounding per sum, of at most u (|a| + |b|)
    return total, bound


def _up_data(B, h, w, ldx, used, exact, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randint(-127, 128, (B, h, w, ldx)) / 256.0 if exact else rng.normal(size=(B, h, w, ldx))).astype(F32)
    x[..., used:] = HUGE
    return x


# B, h, w, H, W, C, G, ldx, ldy, flags
UP_EXACT = [
    (2, 5, 5, 9, 9, 4, 1, 8, 12, 0),                               # scale 1/2
    (2, 3, 3, 9, 9, 68, 1, 72, 100, UP_RELU),                      # scale 1/4
    (2, 9, 9, 5, 5, 4, 1, 4, 8, 0),                                # down, scale 2
    (2, 7, 7, 7, 7, 4, 3, 16, 8, UP_RELU),                         # identity, three groups
    (2, 5, 3, 1, 9, 4, 1, 8, 12, 0),                               # H == 1: scale 0, row 0 is read
    (1, 5, 5, 1, 1, 4, 1, 8, 12, 0),                               # B * H == 1, W == 1: pixel [0, 0]
    (2, 1, 1, 9, 5, 68, 1, 72, 100, 0),                            # every output equals the one input
    (2, 1, 5, 3, 9, 4, 1, 4, 8, UP_RELU),                          # h == 1
    (2, 5, 1, 9, 3, 4, 1, 8, 4, 0),                                # w == 1
    (1, 16, 3, 31, 5, 4, 1, 8, 12, 0),                             # B * H == 31, scale 1/2
    (1, 5, 5, 33, 9, 68, 3, 208, 72, UP_RELU),                     # B * H == 33 (a second group of 32 grid rows), scale 1/8
    (2, 9, 5, 33, 9, 4, 1, 8, 12, UP_ACCUM),                       # B * H == 66
    (2, 5, 5, 9, 9, 4, 3, 16, 12, UP_RELU | UP_ACCUM),
]
UP_GENERAL = [
    (2, 8, 10, 15, 20, 68, 1, 72, 100, 0),
    (2, 8, 10, 15, 20, 4, 3, 16, 8, UP_RELU | UP_ACCUM),
    (2, 7, 19, 20, 31, 280, 1, 284, 288, UP_RELU),                 # W * C / 4 = 2170 > 2048: 9 live workgroups in a grid of 16 columns
    (2, 7, 19, 20, 31, 4, 3, 16, 12, UP_RELU),
]
_UP_ID = lambda c: "b%d_%dx%d_to_%dx%d_c%d_g%d_ldx%d_ldy%d_f%d" % c      # noqa: E731


def _up_inputs(case, exact):
    B, h, w, H, W, C, G, ldx, ldy, flags = case
    x = _up_data(B, h, w, ldx, G * C, exact, sum(case))
    base = _up_data(B * H * W, 1, 1, C, C, exact, sum(case) + 1).reshape(-1, C) if flags & UP_ACCUM else None
    return x, base


def _up(x, case, y, ysp=None, flags=None):
    L = _L()
    B, h, w, H, W, C, G, ldx, ldy, f = case
    f = f if flags is None else flags
    L.check(L.lib().vidc_upsample_bilinear_ac(L.ptr(x), y.ptr(), B, h, w, C, ldx, H, W, ldy, f | ((G << 8) if G > 1 else 0), ysp, L.current_stream()),
            "upsample")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("case", UP_EXACT, ids=_UP_ID)
def test_upsample_exact(case):
    B, h, w, H, W, C, G, ldx, ldy, flags = case
    x, base = _up_inputs(case, True)
    want, _ = _up_expect(x, base, H, W, C, G, flags)
    y = _Rows(B * H * W, C, ldy, base=base)
    _up(_dev(x), case, y)
    got = y.values()
    assert np.array_equal(got.astype(np.float64), want), np.argwhere(got != want)[:4]
    if h == 1 and w == 1:
        assert np.array_equal(got.reshape(B, H * W, C), np.broadcast_to(want.reshape(B, H * W, C)[:, :1], (B, H * W, C)))


@gpu
@pytest.mark.parametrize("case", UP_GENERAL, ids=_UP_ID)
def test_upsample_general(case):
    B, h, w, H, W, C, G, ldx, ldy, flags = case
    x, base = _up_inputs(case, False)
    want, bound = _up_expect(x, base, H, W, C, G, flags)
    y = _Rows(B * H * W, C, ldy, base=base)
    _up(_dev(x), case, y)
    _hold("upsample " + _UP_ID(case), y.values(), want, bound)


@gpu
def test_upsample_split_image_with_and_without_the_f32_store():
    case = (2, 5, 5, 9, 9, 68, 1, 72, 96, UP_RELU)
    B, h, w, H, W, C, G, ldx, ldy, flags = case
    x, _ = _up_inputs(case, True)
    want, _ = _up_expect(x, None, H, W, C, G, flags)
    y, img = _Rows(B * H * W, C, ldy), _split_out(B * H * W, ldy)
    _up(_dev(x), case, y, img.ptr())
    assert np.array_equal(y.values().astype(np.float64), want)
    image = _split_ref(want.astype(F32), ldy)
    assert np.array_equal(_image(img), image)
    y2, img2 = _Rows(B * H * W, C, ldy), _split_out(B * H * W, ldy)
    _up(_dev(x), case, y2, img2.ptr(), flags | UP_NO_F32_OUT)
    assert y2.untouched(), "VIDC_UP_NO_F32_OUT stored fp32 values"
    assert np.array_equal(_image(img2), image)


# ======================================================================================================================================
# head: 1x1 conv to <= 4 channels + upsample
# ======================================================================================================================================
# Cin, Cout, pad, h, w, ldx, H, W
HEAD = [(3, 1, 0, 1, 1, 3, 1, 1), (65, 2, 2, 3, 5, 72, 9, 13), (100, 4, 1, 5, 7, 100, 20, 31), (192, 3, 0, 4, 4, 200, 7, 7)]


@functools.lru_cache(maxsize=None)
def _head_case(Cin, Cout, pad, h, w, ldx):
    g = torch.Generator().manual_seed(Cin * 1000 + Cout * 100 + pad * 10 + h)
    x = torch.randn(2, h, w, ldx, generator=g)
    x[..., Cin:] = HUGE
    wt, bias = torch.randn(Cout, Cin, generator=g) * 0.2, torch.randn(Cout, generator=g)
    xin = x[..., :Cin].permute(0, 3, 1, 2).double()
    low = F.conv2d(xin, wt.double().view(Cout, Cin, 1, 1), bias.double(), padding=pad)
    mag = F.conv2d(xin.abs(), wt.double().abs().view(Cout, Cin, 1, 1), bias.double().abs(), padding=pad)
    return x, wt, bias, low.numpy(), mag.numpy()


@gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Cin,Cout,pad,h,w,ldx,H,W", HEAD, ids=["cin%d_cout%d_pad%d_%dx%d_ldx%d_to_%dx%d" % c for c in HEAD])
def test_head(Cin, Cout, pad, h, w, ldx, H, W, relu):
    L = _L()
    x, wt, bias, low_ref, low_mag = _head_case(Cin, Cout, pad, h, w, ldx)
    hp, wp = h + 2 * pad, w + 2 * pad
    low, y = _Out((2, Cout, hp, wp), torch.float32, float("nan")), _Out((2, Cout, H, W), torch.float32, float("nan"))
    dx, dw, db = x.to(DEV), wt.to(DEV), bias.to(DEV)
    L.check(L.lib().vidc_head_conv1x1_upsample(L.ptr(dx), L.ptr(dw), L.ptr(db), low.ptr(), y.ptr(), 2, h, w, Cin, ldx, Cout, pad, H, W, relu,
                                               L.current_stream()), "head")
    torch.cuda.synchronize()
    got_low, got = low.np(), y.np()
    tag = "cin %d cout %d pad %d" % (Cin, Cout, pad)
    _hold("head_conv " + tag, got_low, low_ref, (-(-Cin // 64) + 8) * U * low_mag)
    ring = np.ones((hp, wp), bool)
    ring[pad:pad + h, pad:pad + w] = False
    assert np.array_equal(got_low[:, :, ring], np.broadcast_to(bias.numpy()[None, :, None], (2, Cout, int(ring.sum())))), "the padded ring is not the bias"
    val, mag, dy, dx = _up_ref(got_low.astype(np.float64).reshape(2 * Cout, hp, wp, 1), H, W)
    if relu:
        val = np.maximum(val, 0.0)
    else:
        assert (val < 0).any() or Cin == 3
    _hold("head_upsample " + tag, got.reshape(-1), val.reshape(-1), (8 * U * mag + 2 * U * dy + 2 * U * dx).reshape(-1))


# ======================================================================================================================================
# CPU tests: the references against torch in float64, the conditions of the exact cases, the host's refusals
# ======================================================================================================================================
@pytest.mark.parametrize("case", UP_EXACT + UP_GENERAL, ids=_UP_ID)
def test_upsample_reference_against_torch(case):
    """The float64 restatement equals F.interpolate(align_corners=True) in float64: bit for bit where the scale is dyadic, and within the
    coordinate term elsewhere (torch takes the scale in float64, the kernel and the restatement in fp32: |scale32 - scale| <= u scale).
    EXACT cases: scale * (out - 1) == in - 1 in fp32, the data sit on a 2^-8 grid and every expected value is an fp32 number."""
    B, h, w, H, W, C, G, ldx, ldy, flags = case
    exact = case in UP_EXACT
    x, base = _up_inputs(case, exact)
    assert ldx >= G * C and ldy >= C and (x[..., G * C:] == HUGE).all()
    for g in range(G):
        xg = x[..., g * C:(g + 1) * C].astype(np.float64)
        val, mag, dy, dx = _up_ref(xg, H, W)
        ref = F.interpolate(torch.from_numpy(xg).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        if exact:
            assert np.array_equal(val, ref)
        else:
            assert (np.abs(val - ref) <= 2 * U * (dy + dx) + 1e-15 * mag).all() and (dy > 0).any() and (dx > 0).any()
        assert (mag >= np.abs(val)).all()
    if exact:
        for n_in, n_out in ((h, H), (w, W)):
            scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
            assert float(scale) * (n_out - 1) == (n_in - 1 if n_out > 1 else 0) and float(scale) * 1024 == int(float(scale) * 1024)
        assert np.array_equal(x[..., :G * C] * 256, np.round(x[..., :G * C] * 256))
        want, _ = _up_expect(x, base, H, W, C, G, flags)
        assert np.array_equal(want.astype(F32).astype(np.float64), want)
        if flags & UP_RELU:
            assert (_up_expect(x, base, H, W, C, G, flags & ~UP_RELU)[0] != want).any()
    if G > 1 and flags & UP_RELU:                                  # ReLU per group differs from a ReLU of the sum
        per, _ = _up_expect(x, None, H, W, C, G, UP_RELU)
        assert (np.abs(per - np.maximum(_up_expect(x, None, H, W, C, G, 0)[0], 0)) > 1e-3).any()


def test_upsample_cases_reach_every_axis():
    cases = UP_EXACT + UP_GENERAL
    assert {c[5] for c in cases} >= {4, 68} and {1, 31, 33, 66} <= {c[0] * c[3] for c in cases}
    assert any(c[4] * c[5] // 4 > 2048 for c in cases) and any(c[7] > c[6] * c[5] and c[8] > c[5] and c[7] != c[8] for c in cases)
    assert any(c[3] < c[1] for c in cases) and {c[6] for c in cases} == {1, 3}
    assert all(c[0] == 2 or c[0] * c[3] in (1, 31, 33) for c in cases)


def test_stem_and_head_references():
    """fp32 torch on the CPU lies within the counted bounds of the float64 references (any order of summation does); every axis value the
    cases must reach is there; conv(|x|, |w|) is nowhere zero."""
    for H, W, Cin, Cout, relu, ldy in STEM:
        x, w, ref, mag = _stem_case(H, W, Cin, Cout)
        y32 = F.conv2d(x, w, None, 2, 1).permute(0, 2, 3, 1).reshape(-1, Cout).numpy()
        assert (np.abs(y32 - ref) <= (9 * Cin + 2) * U * mag).all() and (mag > 0).all() and ref.shape[0] == 2 * ((H + 1) // 2) * ((W + 1) // 2)
        assert ldy in (Cout, _wide(Cout))
    assert {c[:2] for c in STEM} == {(3, 3), (4, 6), (5, 127), (5, 129), (7, 258)} and {c[2] for c in STEM} == {1, 3}
    assert {c[3] for c in STEM} == {1, 32, 64, 100} and {c[4] for c in STEM} == {0, 1} and (5, 129, 3, 100, 0, 160) in STEM
    assert [_wide(c) for c in (1, 32, 64, 100)] == [64, 96, 128, 160]
    for Cin, Cout, pad, h, w, ldx, H, W in HEAD:
        x, wt, bias, low, mag = _head_case(Cin, Cout, pad, h, w, ldx)
        low32 = F.conv2d(x[..., :Cin].permute(0, 3, 1, 2), wt.view(Cout, Cin, 1, 1), bias, padding=pad).numpy()
        assert (np.abs(low32 - low) <= (Cin + 1) * U * mag).all()
        assert low.shape == (2, Cout, h + 2 * pad, w + 2 * pad) and (low[:, :, 0, 0] == bias.numpy().astype(np.float64)).all() == (pad > 0)


def test_pool_inputs_and_split_restatement():
    for H, W, C, ldx, ldy in POOL:
        x, ref = _pool_case(H, W, C, ldx)
        assert not torch.isnan(x).any() and np.isneginf(ref[0]).all() and np.isfinite(ref).any() and ref.shape == (2 * ((H + 1) // 2) * ((W + 1) // 2), C)
    assert -(-(33 * 280 // 4) // 256) == 10                        # (6, 65, 280): 10 live workgroups in a row of 16
    v = np.array([[1.0, -1.0 / 3, 3.14159274, 0.0, 65504.0, 1e-30, -2.5, 1 + 2.0 ** -8]], F32)
    img = _split_ref(v, 32, 8).reshape(1, 1, 2, 32)
    hi, lo = img[0, 0, 0, 8:16].astype(np.uint32) << 16, img[0, 0, 1, 8:16].astype(np.uint32) << 16
    back = hi.view(F32).astype(np.float64) + lo.view(F32).astype(np.float64)
    assert (np.abs(back - v[0]) <= np.abs(v[0]) * 2.0 ** -16).all() and hi.view(F32)[7] == 1.0 and lo.view(F32)[7] == F32(2.0 ** -8)      # RNE: the tie goes to even
    assert (np.delete(img.reshape(-1), np.r_[8:16, 40:48]) == 0xFFFF).all()


@pytest.fixture(scope="module")
def lib():
    L = _L()
    L.build()
    return L.lib()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    p = 4096                                                       # never dereferenced: every call below is refused first
    stem = lambda x=p, y=p, Cin=3, H=5, Cout=32, ldy=96, ysp=None, ch0=0: lib.vidc_stem_conv3x3s2(x, p, y, 2, Cin, H, 9, Cout, ldy, 1, ysp, ch0, None)      # noqa: E731
    shape = [stem(Cin=2), stem(H=2), stem(ldy=31), stem(ysp=p, ldy=40), stem(ysp=p, ch0=-32)]
    null = [stem(y=None), stem(x=None)]
    # the split image is the whole [.., ldy] tensor's: a slice that ends behind the row would be stored into the next pixel's columns
    shape += [stem(ysp=p, ch0=96), stem(ysp=p, ch0=65), stem(ysp=p, y=None, ch0=65), stem(ysp=p, Cout=64, ldy=64, ch0=32)]
    shape += [lib.vidc_stem_conv3x3s2_warped(p, p, p, p, 2, 5, 9, 32, 96, 1, p, 65, 4.0, 2.0, 0, None)]
    null += [lib.vidc_stem_conv3x3s2_warped(p, None, p, p, 2, 5, 9, 32, 96, 1, None, 0, 4.0, 2.0, 0, None)]
    pool = lambda B=2, H=7, C=8, ldx=8, ldy=32, y=p, ysp=None: lib.vidc_maxpool3x3s2(p, y, B, H, 9, C, ldx, ldy, ysp, None)      # noqa: E731
    shape += [pool(C=6), pool(ldx=10), pool(C=12, ldx=8), pool(C=36, ldx=36), pool(C=8, ldy=36, ysp=p), pool(B=65536, H=1)]
    null += [pool(y=None)]
    up = lambda B=2, H=9, C=8, ldx=8, ldy=32, flags=0, ysp=None: lib.vidc_upsample_bilinear_ac(p, p, B, 5, 5, C, ldx, H, 9, ldy, flags, ysp, None)      # noqa: E731
    shape += [up(flags=UP_NO_F32_OUT), up(flags=3 << 8, ldx=16), up(C=6), up(B=2, H=32753), up(ldy=40, ysp=p)]
    head = lambda Cout=1, low=p: lib.vidc_head_conv1x1_upsample(p, p, p, low, p, 2, 3, 5, 64, 64, Cout, 1, 9, 13, 1, None)      # noqa: E731
    shape += [head(0), head(5)]
    null += [head(low=None)]
    assert shape == [ERR_SHAPE] * len(shape), shape
    assert null == [ERR_NULL] * len(null), null
