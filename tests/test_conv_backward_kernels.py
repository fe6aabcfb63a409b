"""The conv backward of torch.ops.vidc, kernel by kernel, at the smallest shapes that reach each branch: vidc_conv_wgrad, vidc_stem_wgrad,
vidc_stem_conv3x3s2_backward_data, vidc_affine_act_backward, the data-gradient weight layouts and ops.conv_backward_data; then the two conv
operators with ill-conditioned epilogues (per-channel scales down to 1e-30 and 0 beside shifts of about +-1).

Kernels are called through the C ABI, or through the ops.* wrapper where it adds nothing but allocation.  References are float64, read only
the fp32 inputs of the call and are plain index-for-index restatements (a CPU test holds each against torch.autograd in float64).  Bounds are
elementwise forward-error bounds built from the reference's own float64 magnitudes (u = 2^-24), never from the kernel's output or a fraction
of a tensor's maximum; where the magnitude is 0 the result must be 0.  Pure data movement is compared bit for bit.  Inputs with ld > C carry
NaN in the gap, outputs a sentinel that must survive.

Counted roundings behind each factor (reading csrc/train.hip; [measured] = the largest error / bound seen on MI355X, profiles/EXPERIMENTS.md):
  conv wgrad       (n + 2) u S|dy x|   n = rows of the longest pixel chunk (<= 1024, wgrad_rows_per_chunk): one fp32 MFMA accumulation per
                                       row (the product and the sum round once each at worst: n + 1 over the chain), then the chunks in
                                       fp64 and one rounding to fp32                                                     [0.27]
  stem wgrad       2 u S|dy x|         fp32 x fp32 products are exact in fp64, the fp64 sums carry 2^-53, one rounding    [0.48]
  stem dgrad       (n + 1) u S|g w|    n = 4 taps x Cout fmaf calls in one chain (the most an input pixel has), one rounding each; + 1
                                       for the second-order terms of the chain                                           [0.16]
  affine dc        1 u |g scale|       one fp32 multiply                                                                  [1.00]
  affine dshift    2 u S|g|            fp64 sum, one rounding                                                             [0.39]
  affine dscale    4 u S|g c|          c = fl(fl(y - shift) / scale) is an fp32 value (2 u), the sum fp64, one rounding;
                   2 u S|g c|          where c is read from c_raw (no arithmetic on it)                                   [0.38]
  dx, precision 0  (K + 2) u S|dc w|   K = Cout x taps terms in one fp32 chain (any order, any split of K has no more), identity epilogue
                                                                                                                          [0.05]
  dx, precision 1  (3 K + 200) u S|dc w|   split bf16: a = ah + al + ra with |a - ah| <= 2^-9 |a| and |ra| <= 2^-9 |a - ah| <= 2^-18 |a|,
                                       the same for w.  The kernel adds ah wh + ah wl + al wh and drops al wl (<= 2^-18 |a w|); the two
                                       residuals lose ra w and a rw (2^-18 |a w| each, second order aside): 3 x 2^-18 = 192 u per term,
                                       200 with the second-order terms.  The three partial products are exact in fp32 (8 x 8 bits) and
                                       sit in one fp32 chain of 3 K terms whose magnitudes sum to (1 + 2^-8) S|a w|.      [0.18]
No factor had to be raised after the measurement.

The operator level (section 5) uses `_compare` of tests/test_torch_ops_autograd.py unchanged: float64 reference, bar = 4 x the deviation of
the same restatement in float32 on the CPU.  It is here because affine_act_bwd_kernel rebuilds c = (y - shift) / scale, whose error grows
like |shift / (scale c)|: with a scale of 2^-10 beside a shift of 1 dscale was off by 1e-5 of its size, with 1e-30 by all of it.  Such
channels (|shift| > 4 |scale|, torch_ops.affine_reads_raw) now read c from the identity-epilogue re-run like the channels with scale 0.
Measured on MI355X, conv2d_bn_act 3x3, shifts of about +-1, dscale, max deviation / max |dscale| over the channels of one scale:
  scale     float32 CPU   bar (4 x)   ours, c rebuilt everywhere   ours, with the rule
  1         5.2e-08       2.1e-07     1.4e-07                      1.4e-07  (rebuilt)
  2^-2      1.7e-07       6.9e-07     1.0e-07                      1.1e-07  (rebuilt where |shift| <= 1)
  2^-3      1.1e-07       4.3e-07     4.2e-08                      6.2e-08  (c_raw from here on)
  2^-6      1.6e-07       6.3e-07     6.5e-07                      9.8e-08
  2^-10     2.0e-07       7.9e-07     1.1e-05                      1.1e-07
  2^-20     2.7e-07       1.1e-06     2.5e-02                      1.3e-07
  1e-30     1.1e-07       4.3e-07     3.6e-01                      7.1e-08
(the 1x1 and the dilated operator measured alike: 6.9e-01 / 3.1e-01 at 1e-30 before, at most 3.7e-07 after; profiles/EXPERIMENTS.md)
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402
from test_torch_ops_autograd import _compare, _nchw, _nhwc  # noqa: E402  (the harness that file's header describes)

from vi_depth_completion_amd import synthetic as S  # noqa: E402
from vi_depth_completion_amd import torch_ops as T  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
V = torch.ops.vidc
U = 2.0 ** -24
F64 = torch.float64
SENTINEL = -7777.0
NAN = float("nan")


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def ref_wgrad(dy, x, KH, KW, stride, pad):
    """dw[co][ci][kh][kw] = S_{b,oy,ox} dy[b][co][oy][ox] * x[b][ci][oy*stride - pad + kh][ox*stride - pad + kw] (0 outside the image), and the
    same sum over absolute values.  dy (B,Cout,Ho,Wo), x (B,Cin,H,W)."""
    dy, x = dy.to(F64), x.to(F64)
    B, Co, Ho, Wo = dy.shape
    _b, Ci, H, W = x.shape
    xp = torch.zeros(B, Ci, H + 2 * pad, W + 2 * pad, dtype=F64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    dw, mag = torch.zeros(Co, Ci, KH, KW, dtype=F64), torch.zeros(Co, Ci, KH, KW, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            win = xp[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            dw[:, :, kh, kw] = torch.einsum("bohw,bchw->oc", dy, win)
            mag[:, :, kh, kw] = torch.einsum("bohw,bchw->oc", dy.abs(), win.abs())
    return dw, mag


def ref_dgrad(dy, w, H, W, stride, pad):
    """dx[b][ci][oy*stride - pad + kh][ox*stride - pad + kw] += dy[b][co][oy][ox] * w[co][ci][kh][kw], the part inside H x W, and the same with
    absolute values.  dy (B,Cout,Ho,Wo), w OIHW."""
    dy, w = dy.to(F64), w.to(F64)
    B, Co, Ho, Wo = dy.shape
    _co, Ci, KH, KW = w.shape
    Hp, Wp = max(H + 2 * pad, (Ho - 1) * stride + KH), max(W + 2 * pad, (Wo - 1) * stride + KW)
    dx, mag = torch.zeros(B, Ci, Hp, Wp, dtype=F64), torch.zeros(B, Ci, Hp, Wp, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            dx[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] += torch.einsum("bohw,oc->bchw", dy, w[:, :, kh, kw])
            mag[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] += torch.einsum("bohw,oc->bchw", dy.abs(), w[:, :, kh, kw].abs())
    return dx[:, :, pad:pad + H, pad:pad + W], mag[:, :, pad:pad + H, pad:pad + W]


def ref_affine(dy, y, scale, shift, relu, c_raw, raw):
    """dc = mask dy scale, dshift = S mask dy, dscale = S mask dy c over the rows; mask = (y > 0) under ReLU; c = c_raw in the channels `raw`
    names, (y - shift) / scale elsewhere.  Rows [M][C]."""
    dy, y, scale, shift = dy.to(F64), y.to(F64), scale.to(F64), shift.to(F64)
    g = dy * (y > 0).to(F64) if relu else dy
    c = (y - shift) / torch.where(raw, torch.ones_like(scale), scale)
    if c_raw is not None:
        c = torch.where(raw, c_raw.to(F64), c)
    else:
        c = torch.where(raw, torch.zeros_like(c), c)
    return dict(dc=g * scale, dc_mag=(g * scale).abs(), dshift=g.sum(0), dshift_mag=g.abs().sum(0), dscale=(g * c).sum(0), dscale_mag=(g * c).abs().sum(0))


def ref_dgrad_layout(w, unit):
    """wp[ci][co / unit][KH-1-kh][KW-1-kw][co % unit] = w[co][ci][kh][kw] (csrc/train.hip, `dgrad helpers`)."""
    co, ci, kh, kw = w.shape
    return w.reshape(co // unit, unit, ci, kh, kw).flip(3, 4).permute(2, 0, 3, 4, 1).contiguous()


def ref_split_bits(v):
    """Units of 32 fp32 values -> [32 x hi | 32 x lo] bf16 bit patterns, hi = RNE(v), lo = RNE(v - hi) (vidc::split_bf16)."""
    v = v.float().reshape(-1, 32)
    return torch.stack([R.bits(v), R.bits(v - R.rounded(v))], 1)


def _raw_channels(scale, shift, c_raw_given, all_raw):
    """The channels of vidc_affine_act_backward that read c_raw: every one with all_raw, else scale == 0 and, when c_raw is given,
    |shift| > 4 |scale| (torch_ops.affine_reads_raw, the expression the kernel evaluates)."""
    if all_raw:
        return torch.ones_like(scale, dtype=torch.bool)
    return T.affine_reads_raw(scale, shift) if c_raw_given else scale == 0


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rows(t, ld, fill=NAN):
    """t [M][C] as device rows of stride ld; the gap holds `fill`."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)


def _nhwc_rows(t):
    """(B,C,H,W) -> rows [B*H*W][C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


RATIOS = {}


def _within(name, got, want, mag, factor, where):
    """|got - want| <= factor * u * mag, elementwise; keeps the largest error / bound ratio seen per quantity."""
    got = got.to(F64).cpu()
    err = (got - want).abs()
    bound = factor * U * mag
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if bool(torch.isfinite(got).all()) else math.inf
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    ok = err <= bound
    if not bool(ok.all()):
        i = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf).flatten()))
        raise AssertionError("%s %s: error / bound = %.3g at flat index %d (got %r, want %r, bound %.3e); %d of %d outside" % (
            name, where, worst, i, float(got.flatten()[i]), float(want.flatten()[i]), float(bound.flatten()[i]), int((~ok).sum()), ok.numel()))


def _report(what):
    print("\n[%s] largest error / bound so far: %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items()))))


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _out_size(n, k, stride, pad):
    return (n + 2 * pad - (k - 1) - 1) // stride + 1


# ---- 1. vidc_conv_wgrad -------------------------------------------------------------------------------------------------------------------
def _wgrad_rows_per_chunk(M, Cout, Cin, taps):
    """wgrad_rows_per_chunk of csrc/train.hip restated."""
    tiles = ((Cout + 127) // 128) * ((Cin + 127) // 128) * taps
    chunks = max((1024 + tiles - 1) // tiles, 1)
    rows = min(max((M + chunks - 1) // chunks, 256), 1024)
    return (rows + 7) // 8 * 8


# (B, H, W, Cin, Cout, KH, KW, stride, pad, ldx - Cin, lddy - Cout, pixel chunks): the branch each one is for
WGRAD_CASES = {
    "m1_1x1": (1, 1, 1, 4, 4, 1, 1, 1, 0, 0, 0, 1),                  # M = 1: seven of the eight row lanes of the only step are past m_hi
    "m1_3x3_all_taps_but_one_outside": (1, 1, 1, 4, 4, 3, 3, 1, 1, 4, 8, 1),
    "m297_two_chunks_36x68": (3, 9, 11, 68, 36, 3, 3, 1, 1, 4, 8, 2),     # chunk 2 starts at row 256 = image 2, row 5, column 3; it has 41 rows (41 % 8 != 0);
    #                                                                       Cout 36 / Cin 68 ragged against the 32-lane and 64-wave tiles; ldx > Cin, lddy > Cout
    "m297_1x1_132x130": (3, 9, 11, 130, 132, 1, 1, 1, 0, 0, 0, 2),        # a second 128-workgroup tile in both channel dimensions, 4 and 2 channels wide
    "m297_3x3_128x128": (3, 9, 11, 128, 128, 3, 3, 1, 1, 4, 8, 2),        # full tiles
    "wo1": (4, 9, 1, 4, 4, 3, 3, 1, 1, 0, 0, 1),                          # Wo = 1: the ox walk wraps eight rows per step
    "wo3_two_chunks": (14, 7, 3, 4, 36, 3, 3, 1, 1, 4, 0, 2),             # Wo = 3, M = 294: chunk 2 starts at image 12, row 1, column 1
    "ho1": (2, 3, 7, 4, 4, 3, 3, 1, 0, 0, 8, 1),                          # Ho = 1 (pad 0): every step crosses images
    "k1x3_pad0": (3, 9, 13, 68, 36, 1, 3, 1, 0, 4, 8, 2),                 # KH != KW
    "k1x3_pad1": (3, 7, 11, 4, 4, 1, 3, 1, 1, 0, 0, 2),                   # ... with pad > (KH-1)/2: output rows 0 and 8 read nothing but padding
    "k3x3_pad0": (3, 11, 13, 4, 36, 3, 3, 1, 0, 0, 8, 2),
    "k3x3_pad2": (3, 7, 9, 68, 4, 3, 3, 1, 2, 4, 0, 2),                   # pad > (k-1)/2
    "s2_1x1_odd": (3, 9, 11, 68, 36, 1, 1, 2, 0, 4, 8, 1),                # stride 2 at both parities of H and W; M = 90 (90 % 8 != 0)
    "s2_1x1_even": (3, 10, 12, 68, 36, 1, 1, 2, 0, 0, 0, 1),
    "s2_3x3_odd": (3, 9, 11, 68, 36, 3, 3, 2, 1, 4, 8, 1),
    "s2_3x3_even": (3, 10, 12, 4, 4, 3, 3, 2, 1, 0, 0, 1),
}


def _wgrad_data(case):
    B, H, W, Cin, Cout, KH, KW, stride, pad = WGRAD_CASES[case][:9]
    Ho, Wo = _out_size(H, KH, stride, pad), _out_size(W, KW, stride, pad)
    seed = sum(ord(ch) for ch in case)
    return _randn(seed, B, Cin, H, W), _randn(seed + 1, B, Cout, Ho, Wo), Ho, Wo


@gpu
@pytest.mark.parametrize("case", sorted(WGRAD_CASES))
def test_conv_wgrad(case):
    """vidc_conv_wgrad against ref_wgrad under (n + 2) u S|dy x|; the scratch size names the chunk count the case is meant to have; two runs
    give the same bits (scratch pre-filled with NaN, dw with a sentinel)."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, H, W, Cin, Cout, KH, KW, stride, pad, gx, gdy, chunks = WGRAD_CASES[case]
    x, dy, Ho, Wo = _wgrad_data(case)
    M, taps = B * Ho * Wo, KH * KW
    rows = _wgrad_rows_per_chunk(M, Cout, Cin, taps)
    assert (M + rows - 1) // rows == chunks, (M, rows)
    nbytes = lib.vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, Cout, Cin, KH, KW)
    assert nbytes == chunks * taps * Cout * Cin * 4, "%s no longer has %d pixel chunks" % (case, chunks)
    xd, dyd = _rows(_nhwc_rows(x), Cin + gx), _rows(_nhwc_rows(dy), Cout + gdy)
    runs = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, KH, KW), SENTINEL, device=DEV)
        sc = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        L.check(lib.vidc_conv_wgrad(L.ptr(dyd), L.ptr(xd), L.ptr(dw), B, H, W, Cin, Cin + gx, Ho, Wo, Cout, Cout + gdy, KH, KW, stride, pad, L.ptr(sc),
                                    L.current_stream()), "conv_wgrad")
        torch.cuda.synchronize()
        runs.append(dw.cpu())
    want, mag = ref_wgrad(dy, x, KH, KW, stride, pad)
    _within("conv_wgrad", runs[0], want, mag, min(rows, M) + 2, case)
    assert _same_bits(runs[0], runs[1]), "%s: two runs differ" % case
    _report("conv wgrad %s" % case)


# ---- 2. the stem ---------------------------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout): Cin 1 and 3; 1x1 and 2x3 maps (every row takes the per-tap border path); odd and even sizes; five 9x11 images = 150
# rows of 30 per image, which the 64-row chunks cut inside images 2 and 4
STEM_CASES = [(2, cin, h, w, co) for cin in (1, 3) for (h, w) in ((1, 1), (2, 3), (5, 7), (6, 8)) for co in (4, 64)] + [(5, 3, 9, 11, 64), (5, 1, 9, 11, 4)]


def _stem_data(B, Cin, H, W, Cout):
    seed = 10000 * B + 1000 * Cin + 100 * H + 10 * W + Cout
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, dy, w = _randn(seed, B, Cin, H, W), _randn(seed + 1, B, Cout, Ho, Wo), _randn(seed + 2, Cout, Cin, 3, 3) * 0.3
    y = _randn(seed + 3, B, Cout, Ho, Wo)
    flat = y.reshape(-1)
    flat[0::5] = 0.0                # closed gates at exactly 0 ...
    flat[1::7] = -0.0               # ... and at -0.0
    return x, dy, w, y, Ho, Wo


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout", STEM_CASES, ids=["b%d_c%d_%dx%d_o%d" % c for c in STEM_CASES])
def test_stem_backward(B, Cin, H, W, Cout):
    """vidc_stem_wgrad (lddy > Cout) under 2 u S|dy x| and vidc_stem_conv3x3s2_backward_data (lddy != ldy, with and without y) under
    (4 Cout + 1) u S|g w|; the ReLU mask is exactly y > 0 (y holds 0 and -0.0); both twice, same bits."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    x, dy, w, y, Ho, Wo = _stem_data(B, Cin, H, W, Cout)
    where = "B=%d Cin=%d %dx%d Cout=%d" % (B, Cin, H, W, Cout)
    lddy, ldy = Cout + 4, Cout + 8
    dyd, yd, xd, wd = _rows(_nhwc_rows(dy), lddy), _rows(_nhwc_rows(y), ldy), x.to(DEV), w.to(DEV)
    nbytes = lib.vidc_stem_wgrad_scratch_bytes(B, Cin, H, W, Cout)
    assert nbytes == ((B * Ho * Wo + 63) // 64) * Cout * Cin * 9 * 8
    runs = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, 3, 3), SENTINEL, device=DEV)
        sc = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        L.check(lib.vidc_stem_wgrad(L.ptr(dyd), L.ptr(xd), L.ptr(dw), B, Cin, H, W, Cout, lddy, L.ptr(sc), L.current_stream()), "stem_wgrad")
        torch.cuda.synchronize()
        runs.append(dw.cpu())
    want, mag = ref_wgrad(dy, x, 3, 3, 2, 1)
    _within("stem_wgrad", runs[0], want, mag, 2, where)
    assert _same_bits(runs[0], runs[1]), "%s: two stem_wgrad runs differ" % where
    for with_y in (False, True):
        g = dy * (y > 0).float() if with_y else dy
        want, mag = ref_dgrad(g, w, H, W, 2, 1)
        runs = []
        for _ in range(2):
            dx = torch.full((B, Cin, H, W), SENTINEL, device=DEV)
            L.check(lib.vidc_stem_conv3x3s2_backward_data(L.ptr(dyd), L.ptr(yd) if with_y else None, L.ptr(wd), L.ptr(dx), B, Cin, H, W, Cout, lddy, ldy,
                                                          L.current_stream()), "stem dgrad")
            torch.cuda.synchronize()
            runs.append(dx.cpu())
        _within("stem_dgrad", runs[0], want, mag, 4 * Cout + 1, "%s y=%d" % (where, with_y))
        assert _same_bits(runs[0], runs[1]), "%s: two stem dgrad runs differ" % where
    _report("stem %s" % where)


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout", [(2, 3, 5, 7, 64), (5, 1, 9, 11, 4)])
def test_stem_backward_weight_wrapper_masks_with_y(B, Cin, H, W, Cout):
    """ops.stem_conv3x3s2_backward_weight with ReLU = the same float64 reference after masking dy with y > 0 (the masking is exact)."""
    from vi_depth_completion_amd import ops
    x, dy, _w, y, _ho, _wo = _stem_data(B, Cin, H, W, Cout)
    for relu in (True, False):
        got = ops.stem_conv3x3s2_backward_weight(_nhwc(dy).to(DEV), _nhwc(y).to(DEV), x.to(DEV), (Cout, Cin, 3, 3), relu=relu)
        want, mag = ref_wgrad(dy * (y > 0).float() if relu else dy, x, 3, 3, 2, 1)
        _within("stem_wgrad", got, want, mag, 2, "wrapper B=%d Cin=%d %dx%d relu=%d" % (B, Cin, H, W, relu))


# ---- 3. vidc_affine_act_backward --------------------------------------------------------------------------------------------------------------
# (M, C): one row; one row past a chunk of 32 (rows_for) and a second channel block of 4; 9 chunks and three channel blocks, the last of 4
AFFINE_SHAPES = [(1, 4), (33, 68), (257, 132)]


def _rows_for(M, C):
    r = (M * ((C + 63) // 64) + 511) // 512
    r = (r + 15) // 16 * 16
    return min(max(r, 32), 256)


def _affine_data(M, C):
    """Channels 0 and C-1: scale exactly 0 with a positive and a negative shift (y == relu?(shift) in every row).  With C >= 8, channel 2:
    scale 2^-10 beside shift 1 (ill-conditioned), channel 5: scale -0.75.  c_raw is unrelated to y."""
    seed = 100 * M + C
    scale, shift = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed)), 0.1 * _randn(seed + 1, C)
    y, dy, c_raw = _randn(seed + 2, M, C), _randn(seed + 3, M, C), _randn(seed + 4, M, C)
    flat = y.reshape(-1)
    flat[0::5] = 0.0
    flat[1::7] = -0.0
    if C >= 8:
        scale[2], shift[2], scale[5] = 2.0 ** -10, 1.0, -0.75
    scale_z, shift_z = scale.clone(), shift.clone()
    scale_z[0], shift_z[0], scale_z[C - 1], shift_z[C - 1] = 0.0, 0.5, 0.0, -0.5
    return dict(scale=scale, shift=shift, scale_z=scale_z, shift_z=shift_z, y=y, dy=dy, c_raw=c_raw)


def _run_affine(L, d, M, C, scale, shift, y, relu, c_raw, all_raw, strides):
    lib = L.lib()
    lddy, ldy, ldc, lddc = strides
    dyd, yd = _rows(d["dy"], lddy), _rows(y, ldy)
    cd = _rows(c_raw, ldc) if c_raw is not None else None
    dc = torch.full((M, lddc), SENTINEL, device=DEV)
    dscale, dshift = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    sc = torch.full((lib.vidc_train_scratch_bytes(M, C),), 0xFF, dtype=torch.uint8, device=DEV)
    scale_d, shift_d = scale.to(DEV), shift.to(DEV)
    L.check(lib.vidc_affine_act_backward(L.ptr(dyd), L.ptr(yd), L.ptr(cd), L.ptr(scale_d), L.ptr(shift_d), L.ptr(dc), L.ptr(dscale), L.ptr(dshift),
                                         M, C, lddy, ldy, -ldc if all_raw else ldc, lddc, relu, L.ptr(sc), L.current_stream()), "affine_act_backward")
    torch.cuda.synchronize()
    return dc.cpu(), dscale.cpu(), dshift.cpu()


@gpu
@pytest.mark.parametrize("M,C", AFFINE_SHAPES, ids=["%dx%d" % s for s in AFFINE_SHAPES])
def test_affine_act_backward(M, C):
    """dc, dscale, dshift relative to the call's own inputs, ReLU on and off, dense rows and four different row strides, in four modes:
    c_raw == NULL without a zero scale (every channel rebuilt, the ill-conditioned one too); c_raw given with two zero-scale channels (those
    and the ill-conditioned channel read it, the rest is rebuilt -- and has the bits of the call without c_raw); all_raw; and zero scales
    without c_raw (c = 0 there)."""
    from vi_depth_completion_amd import _lib as L
    d = _affine_data(M, C)
    assert (M + _rows_for(M, C) - 1) // _rows_for(M, C) == {1: 1, 33: 2, 257: 9}[M]
    for relu in (0, 1):
        for strides in ((C, C, C, C), (C + 4, C + 8, C + 12, C + 16)):
            results = {}
            for mode in ("null", "zeros+raw", "all_raw", "zeros"):
                scale, shift = (d["scale"], d["shift"]) if mode in ("null", "all_raw") else (d["scale_z"], d["shift_z"])
                y = d["y"].clone()
                if mode in ("zeros+raw", "zeros"):           # what the forward leaves in a channel with scale 0
                    y[:, 0], y[:, C - 1] = shift[0], (shift[C - 1].clamp_min(0.0) if relu else shift[C - 1])
                c_raw = None if mode in ("null", "zeros") else d["c_raw"]
                raw = _raw_channels(scale, shift, c_raw is not None, mode == "all_raw")
                if mode == "null":
                    assert not bool(raw.any())
                if mode == "zeros+raw":
                    assert int(raw.sum()) == (3 if C >= 8 else 2) and not bool(raw[1])
                where = "(%d, %d) relu=%d strides=%s %s" % (M, C, relu, strides, mode)
                ref = ref_affine(d["dy"], y, scale, shift, relu, c_raw, raw)
                dc, dscale, dshift = _run_affine(L, d, M, C, scale, shift, y, relu, c_raw, mode == "all_raw", strides)
                _within("affine_dc", dc[:, :C], ref["dc"], ref["dc_mag"], 1, where)
                assert bool((dc[:, C:] == SENTINEL).all()), "%s: the gap of dc was written" % where
                _within("affine_dshift", dshift, ref["dshift"], ref["dshift_mag"], 2, where)
                _within("affine_dscale", dscale, ref["dscale"], ref["dscale_mag"], torch.where(raw, 2.0, 4.0).to(F64), where)
                if relu and mode in ("zeros+raw", "zeros"):      # the channel with scale 0 and a negative shift is fully masked
                    assert float(dscale[C - 1]) == 0.0 and float(dshift[C - 1]) == 0.0 and not bool(dc[:, C - 1].any())
                results[mode] = (dscale, dshift, dc)
            keep = ~_raw_channels(d["scale_z"], d["shift_z"], True, False)       # rebuilt in both calls, same parameters and rows
            for a, b in zip(results["zeros+raw"], results["zeros"]):
                assert _same_bits(a[..., :C][..., keep], b[..., :C][..., keep]), "a rebuilt channel changed bits beside channels that read c_raw"
    _report("affine_act_backward %s" % ((M, C),))


# ---- 4. data-gradient weights and ops.conv_backward_data ---------------------------------------------------------------------------------------
PACK_SHAPES = [(cin, k) for cin in (12, 70) for k in (1, 3)]          # Cin ragged against kPackCi = 8 (3x3) and 64 (1x1)


def _pack_batched(L, items):
    """items: (w, packed, Cout, Cin, KH, KW, kind) with device tensors; one vidc_pack_conv_weights_batched launch over all of them."""
    lib = L.lib()
    arr = (L.PackItem * len(items))()
    begin = 0
    for i, (w, packed, co, ci, kh, kw, kind) in enumerate(items):
        nb = lib.vidc_pack_item_blocks(co, ci, kh, kw, kind)
        assert nb > 0, (co, ci, kh, kw, kind)
        arr[i].w, arr[i].packed, arr[i].Cout, arr[i].Cin, arr[i].KH, arr[i].KW, arr[i].kind, arr[i].block_begin = L.ptr(w), L.ptr(packed), co, ci, kh, kw, kind, begin
        begin += nb
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.check(lib.vidc_pack_conv_weights_batched(L.ptr(dev), len(items), begin, L.current_stream()), "pack_conv_weights_batched")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("kind", [1, 3, 5], ids=["fp32", "split_bf16", "plain_bf16"])
def test_dgrad_weight_layouts_bit_for_bit(kind):
    """The dgrad kinds of vidc_pack_conv_weights_batched, eight weights in one launch at odd offsets of one flat parameter buffer, against
    ref_dgrad_layout (fp32: a copy; split bf16: hi | lo per unit of 32; plain bf16: RNE, units of 64), every bit and the 64 elements behind
    each packed image; the fp32 kind against vidc_pack_conv_weight_dgrad as well."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    unit = 64 if kind == 5 else 32
    shapes = [(co, cin, k) for co in ((64, 128) if kind == 5 else (32, 96)) for cin, k in PACK_SHAPES]
    ws = [_randn(7 * co + cin + k, co, cin, k, k) for co, cin, k in shapes]
    flat = torch.full((sum(w.numel() + 1 for w in ws) + 1,), NAN)
    views, off = [], 1                                           # 4 bytes past the allocation's alignment, then one NaN between parameters
    for w in ws:
        flat[off:off + w.numel()] = w.reshape(-1)
        views.append((off, w.numel()))
        off += w.numel() + 1
    flat_d = flat.to(DEV)
    out_dtype = torch.int16 if kind == 5 else torch.float32
    outs = [torch.full((w.numel() + 64,), -21846 if kind == 5 else SENTINEL, dtype=out_dtype, device=DEV) for w in ws]
    _pack_batched(L, [(flat_d[o:o + n], out, co, cin, k, k, kind) for (o, n), out, (co, cin, k) in zip(views, outs, shapes)])
    for w, out, (co, cin, k) in zip(ws, outs, shapes):
        where = "kind %d, %dx%dx%dx%d" % (kind, co, cin, k, k)
        want = ref_dgrad_layout(w, unit)
        got, tail = out[:w.numel()].cpu(), out[w.numel():].cpu()
        assert bool((tail == (-21846 if kind == 5 else SENTINEL)).all()), "%s: written past the packed image" % where
        if kind == 1:
            assert _same_bits(got, want.reshape(-1)), where
            single, wd = torch.full((w.numel(),), SENTINEL, device=DEV), w.to(DEV)
            L.check(lib.vidc_pack_conv_weight_dgrad(L.ptr(wd), L.ptr(single), co, cin, k, k, L.current_stream()), "pack_conv_weight_dgrad")
            torch.cuda.synchronize()
            assert _same_bits(single.cpu(), want.reshape(-1)), "single entry, " + where
            assert _same_bits(single.cpu(), got), "single entry and batched fp32 kind differ, " + where
        elif kind == 3:
            assert torch.equal(got.view(torch.int16).to(torch.int32).reshape(-1, 2, 32) & 0xFFFF, ref_split_bits(want)), where
        else:
            assert torch.equal(got.to(torch.int32) & 0xFFFF, R.bits(want).reshape(-1)), where


# (k, stride, pad, H, W): 3x3 "same"; stride 2 at both parities; stride 2 padded below "same" (the crop; at 10x12 row 9 and column 11 lie in no
# window); 1x1 stride 2 at both parities; 1x1
DGRAD_CASES = [(3, 1, 1, 9, 11), (3, 2, 1, 9, 11), (3, 2, 1, 10, 12), (3, 2, 0, 9, 11), (3, 2, 0, 10, 12), (1, 2, 0, 9, 11), (1, 2, 0, 10, 12), (1, 1, 0, 9, 11)]
DGRAD_B, DGRAD_CIN, DGRAD_COUT = 2, 32, 64


def _dgrad_data(k, stride, pad, H, W):
    seed = 1000 * k + 100 * stride + 10 * pad + H
    Ho, Wo = _out_size(H, k, stride, pad), _out_size(W, k, stride, pad)
    return _randn(seed, DGRAD_B, DGRAD_COUT, Ho, Wo), _randn(seed + 1, DGRAD_COUT, DGRAD_CIN, k, k) * (2.0 / (DGRAD_COUT * k * k)) ** 0.5


@gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=["k%d_s%d_p%d_%dx%d" % c for c in DGRAD_CASES])
def test_conv_backward_data(case, precision):
    """ops.conv_backward_data against ref_dgrad: (K + 2) u S|dc w| at precision 0, (3 K + 200) u S|dc w| at precision 1 (module docstring),
    K = Cout * taps; an input pixel that no window covers has magnitude 0, so its gradient must be exactly 0."""
    from vi_depth_completion_amd import ops
    k, stride, pad, H, W = case
    dc, w = _dgrad_data(*case)
    want, mag = ref_dgrad(dc, w, H, W, stride, pad)
    if case == (3, 2, 0, 10, 12):
        assert float(mag[:, :, 9].max()) == 0.0 and float(mag[:, :, :, 11].max()) == 0.0 and float(mag[:, :, :9, :11].min()) > 0.0
    if k == 1 and stride == 2:
        assert float(mag[:, :, 1::2].max()) == 0.0 and float(mag[:, :, :, 1::2].max()) == 0.0
    got = ops.conv_backward_data(_nhwc(dc).to(DEV), w.to(DEV), H, W, stride, pad, precision)
    assert got.shape == (DGRAD_B, H, W, DGRAD_CIN) and got.is_contiguous()
    K = DGRAD_COUT * k * k
    _within("dx_p%d" % precision, _nchw(got.cpu()), want, mag, (K + 2) if precision == 0 else (3 * K + 200), "%s precision %d" % (case, precision))
    _report("conv_backward_data %s p%d" % (case, precision))


@gpu
def test_conv_backward_data_refusals():
    from vi_depth_completion_amd import ops
    dc = torch.zeros(1, 9, 11, 64, device=DEV)
    for shape, stride, pad in (((64, 32, 1, 3), 1, 0), ((64, 32, 3, 3), 1, 3), ((64, 32, 3, 3), 2, 2)):       # kh != kw; pad > k-1; strided, 2 pad > k-1
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            ops.conv_backward_data(dc, torch.zeros(shape, device=DEV), 9, 11, stride, pad)


# ---- 5. operator level: ill-conditioned epilogues ----------------------------------------------------------------------------------------------
ILL_SCALES = [1.0, 2.0 ** -3, 2.0 ** -6, 2.0 ** -10, 2.0 ** -20, 1e-30, 0.0]
ILL_OPS = {"3x3": (3, 1, 1), "1x1": (1, 0, 1), "dilated": (3, 2, 2)}           # (k, pad, dilation)
ILL_DELTA = 1e-3


def _ill_case(op, shift_mode, scales=ILL_SCALES):
    """B = 2, 64 -> 32 channels, 9 x 11.  Channel i has scale scales[i % n]; its shift is 0, or about 1 with the sign of (-1)^(i // n), so that
    every scale meets both signs."""
    k = ILL_OPS[op][0]
    x = S.normal01(41, "ill.x", (2, 64, 9, 11)).float()
    w = S.normal01(41, "ill.w." + op, (32, 64, k, k)).float() * (2.0 / (64 * k * k)) ** 0.5
    n = len(scales)
    scale = torch.tensor([scales[i % n] for i in range(32)], dtype=torch.float32)
    if shift_mode == "zero":
        shift = torch.zeros(32)
    else:
        shift = torch.tensor([1.0 if (i // n) % 2 == 0 else -1.0 for i in range(32)]) * (0.9 + 0.2 * S.uniform01(41, "ill.b", (32,)).float())
    return x, w, scale, shift


def _ill_ref(op, relu):
    _k, pad, dil = ILL_OPS[op]

    def ref(x, w, scale, shift):
        pre = F.conv2d(x, w, padding=pad, dilation=dil) * scale[None, :, None, None] + shift[None, :, None, None]
        return (F.relu(pre) if relu else pre), pre
    return ref


def _ill_ours(op, relu):
    _k, pad, dil = ILL_OPS[op]
    if op == "dilated":
        return lambda x, w, s, b: _nchw(V.conv2d_dilated_bn_act(_nhwc(x), w, s, b, pad, dil, relu, 0))
    return lambda x, w, s, b: _nchw(V.conv2d_bn_act(_nhwc(x), w, s, b, 1, pad, relu, 0))


@gpu
@pytest.mark.parametrize("shift_mode", ["pm1", "zero"])
@pytest.mark.parametrize("op", sorted(ILL_OPS))
def test_ill_conditioned_epilogue_gradients(op, shift_mode):
    """dx, dw, dscale, dshift of conv2d_bn_act (3x3, 1x1) and conv2d_dilated_bn_act at precision 0, no ReLU, per-channel scales 1, 2^-3, 2^-6,
    2^-10, 2^-20, 1e-30 and 0 beside shifts of about +-1 or of 0."""
    _compare("ill[%s,shift=%s]" % (op, shift_mode), _ill_ref(op, False), _ill_ours(op, False), _ill_case(op, shift_mode), ["x", "w", "scale", "shift"])


@gpu
def test_ill_conditioned_epilogue_gradients_relu():
    """The same scales beside shifts of about +-1 under ReLU: a channel with a small scale is open (shift > 0) or closed (shift < 0) in every
    row, so the gated share stays under the cap (checked on the CPU below)."""
    _compare("ill[3x3,shift=pm1,relu]", _ill_ref("3x3", True), _ill_ours("3x3", True), _ill_case("3x3", "pm1"), ["x", "w", "scale", "shift"], delta=ILL_DELTA)


def test_ill_conditioned_relu_gates_stay_under_the_cap():
    """The float64 side alone: at most 1 % of the pre-activations of the gated case lie within delta of zero; and the parameters are what the
    case is for -- every scale below 2^-2 beside a shift of about 1 reads c from the re-run, scale 1 does not, nor does any channel with shift 0."""
    x, w, scale, shift = _ill_case("3x3", "pm1")
    pre = _ill_ref("3x3", True)(x.double(), w.double(), scale.double(), shift.double())[1]
    assert (pre.abs() < ILL_DELTA).double().mean().item() <= 0.01
    assert T.affine_reads_raw(scale, shift).tolist() == [s != 1.0 for s in scale.tolist()]
    scale0, shift0 = _ill_case("3x3", "zero")[2:]
    assert T.affine_reads_raw(scale0, shift0).tolist() == [s == 0.0 for s in scale0.tolist()]


def _conv_backward_counting_convs(x, w, scale, shift, dy, relu=False):
    """One forward + backward of conv2d_bn_act (3x3, precision 0); returns the gradients and how often the backward launched ops.conv2d_bn_act
    (the data gradient is one launch; a second one is the identity-epilogue re-run)."""
    from vi_depth_completion_amd import ops
    with torch.enable_grad():
        leaves = [t.clone().requires_grad_() for t in (x, w, scale, shift)]
        out = V.conv2d_bn_act(*leaves, 1, 1, relu, 0)
        launched = []
        real = ops.conv2d_bn_act
        ops.conv2d_bn_act = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
        try:
            grads = torch.autograd.grad((out * dy).sum(), leaves)
        finally:
            ops.conv2d_bn_act = real
    return grads, len(launched)


@gpu
def test_well_conditioned_channels_launch_no_extra_conv_and_keep_their_bits():
    """Parameters like every other test's (scale in [0.5, 1.5], shift 0.1 N(0,1)): the backward launches the data-gradient conv and nothing
    else.  With some channels made ill-conditioned it launches the re-run as well, and dscale, dshift of the untouched channels keep
    their bits."""
    x = _nhwc(S.normal01(43, "mix.x", (2, 64, 9, 11)).float()).to(DEV)
    w = (S.normal01(43, "mix.w", (32, 64, 3, 3)).float() * (2.0 / 576) ** 0.5).to(DEV)
    scale, shift = 0.5 + S.uniform01(43, "mix.s", (32,)).float(), 0.1 * S.normal01(43, "mix.b", (32,)).float()
    dy = S.normal01(43, "mix.dy", (2, 9, 11, 32)).float().to(DEV)
    assert not bool(T.affine_reads_raw(scale, shift).any())
    well, n_well = _conv_backward_counting_convs(x, w, scale.to(DEV), shift.to(DEV), dy)
    assert n_well == 1
    ill_scale, ill_shift = scale.clone(), shift.clone()
    ill = [3, 17, 31]
    ill_scale[ill], ill_shift[ill] = torch.tensor([2.0 ** -10, 1e-30, 0.0]), torch.tensor([1.0, -1.0, 0.25])
    assert T.affine_reads_raw(ill_scale, ill_shift).nonzero().flatten().tolist() == ill
    mixed, n_mixed = _conv_backward_counting_convs(x, w, ill_scale.to(DEV), ill_shift.to(DEV), dy)
    assert n_mixed == 2
    keep = torch.ones(32, dtype=torch.bool)
    keep[ill] = False
    for a, b, name in ((well[2], mixed[2], "dscale"), (well[3], mixed[3], "dshift")):
        assert _same_bits(a.cpu()[keep], b.cpu()[keep]), name


# ---- CPU: the yardsticks themselves ------------------------------------------------------------------------------------------------------------
def _rel(got, want, mag):
    assert bool(((got - want).abs() <= 1e-12 * mag).all()), float(((got - want).abs() / mag.clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", ["m297_two_chunks_36x68", "k1x3_pad1", "k3x3_pad2", "s2_3x3_even", "s2_1x1_odd", "ho1"])
def test_conv_references_agree_with_autograd_in_float64(case):
    """ref_wgrad and ref_dgrad against torch.autograd on F.conv2d in float64, to 1e-12 of the magnitudes the bounds are built from."""
    B, H, W, Cin, Cout, KH, KW, stride, pad = WGRAD_CASES[case][:9]
    x, dy, _ho, _wo = _wgrad_data(case)
    w = _randn(5, Cout, Cin, KH, KW).to(F64).requires_grad_()
    xl = x.to(F64).requires_grad_()
    with torch.enable_grad():
        F.conv2d(xl, w, stride=stride, padding=pad).backward(dy.to(F64))
    dw, dw_mag = ref_wgrad(dy, x, KH, KW, stride, pad)
    _rel(dw, w.grad, dw_mag)
    dx, dx_mag = ref_dgrad(dy, w.detach(), H, W, stride, pad)
    _rel(dx, xl.grad, dx_mag)
    assert bool((dw_mag >= dw.abs() * (1 - 1e-12)).all()) and bool((dx_mag >= dx.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("case", DGRAD_CASES[:1] + DGRAD_CASES[3:6], ids=lambda c: "k%d_s%d_p%d_%dx%d" % c)
def test_dgrad_reference_and_layout_agree_with_autograd_in_float64(case):
    """ref_dgrad at the shapes of test_conv_backward_data; and, for stride 1, the data-gradient layout read back as the forward weights of a conv
    with Cout' = Cin, Cin' = Cout and pad' = k - 1 - pad gives the same dx."""
    k, stride, pad, H, W = case
    dc, w = _dgrad_data(*case)
    xl = torch.zeros(DGRAD_B, DGRAD_CIN, H, W, dtype=F64).requires_grad_()
    with torch.enable_grad():
        F.conv2d(xl, w.to(F64), stride=stride, padding=pad).backward(dc.to(F64))
    dx, mag = ref_dgrad(dc, w, H, W, stride, pad)
    _rel(dx, xl.grad, mag)
    if stride == 1:
        wp = ref_dgrad_layout(w, 32)                                       # [Cin][Cout/32][kh][kw][32]: the forward layout of an OIHW' weight
        w_t = wp.permute(0, 1, 4, 2, 3).reshape(DGRAD_CIN, DGRAD_COUT, k, k)
        _rel(F.conv2d(dc.to(F64), w_t.to(F64), padding=k - 1 - pad), xl.grad, mag)


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(2, 3, 5, 7, 4), (2, 1, 2, 3, 4), (5, 3, 9, 11, 64), (2, 1, 1, 1, 4)])
def test_stem_references_agree_with_autograd_in_float64(B, Cin, H, W, Cout):
    x, dy, w, y, _ho, _wo = _stem_data(B, Cin, H, W, Cout)
    assert bool((y == 0).any()) and bool((torch.signbit(y) & (y == 0)).any())
    xl, wl = x.to(F64).requires_grad_(), w.to(F64).requires_grad_()
    g = dy * (y > 0).float()
    with torch.enable_grad():
        F.conv2d(xl, wl, stride=2, padding=1).backward(g.to(F64))
    _rel(ref_wgrad(g, x, 3, 3, 2, 1)[0], wl.grad, ref_wgrad(g, x, 3, 3, 2, 1)[1])
    _rel(ref_dgrad(g, w, H, W, 2, 1)[0], xl.grad, ref_dgrad(g, w, H, W, 2, 1)[1])


@pytest.mark.parametrize("M,C", AFFINE_SHAPES[1:])
@pytest.mark.parametrize("relu", [0, 1])
def test_affine_reference_agrees_with_autograd_in_float64(M, C, relu):
    """ref_affine against autograd of relu?(c * scale + shift): with y the float64 image of c the rebuilt c is c itself, and a channel with scale
    0 reads it from c_raw = c."""
    d = _affine_data(M, C)
    c = d["c_raw"].to(F64).requires_grad_()
    scale, shift = d["scale_z"].to(F64).requires_grad_(), d["shift_z"].to(F64).requires_grad_()
    with torch.enable_grad():
        pre = c * scale + shift
        y = F.relu(pre) if relu else pre
        y.backward(d["dy"].to(F64))
    raw = d["scale_z"] == 0
    ref = ref_affine(d["dy"], y.detach(), scale.detach(), shift.detach(), relu, c.detach(), raw)
    _rel(ref["dc"], c.grad, ref["dc_mag"])
    _rel(ref["dshift"], shift.grad, ref["dshift_mag"])
    # (the quotient has a conditioning of its own in float64 as well: |shift / scale| per unit of y's rounding, 1024 in channel 2)
    open_ = (y.detach() > 0).to(F64) if relu else torch.ones_like(y.detach())
    cond = (shift.detach() / torch.where(raw, torch.ones_like(raw, dtype=F64), scale.detach())).abs().masked_fill(raw, 0.0)
    _rel(ref["dscale"], scale.grad, ref["dscale_mag"] + (d["dy"].to(F64) * open_).abs().sum(0) * cond)
    assert int(raw.sum()) == 2


def test_wgrad_cases_have_the_chunks_they_are_for():
    """The restated wgrad_rows_per_chunk gives every case its chunk count, and the two-chunk cases start their second chunk inside an image and
    inside an image row, with a row count that is no multiple of 8."""
    for case, (B, H, W, Cin, Cout, KH, KW, stride, pad, _gx, _gdy, chunks) in WGRAD_CASES.items():
        Ho, Wo = _out_size(H, KH, stride, pad), _out_size(W, KW, stride, pad)
        M = B * Ho * Wo
        rows = _wgrad_rows_per_chunk(M, Cout, Cin, KH * KW)
        assert (M + rows - 1) // rows == chunks, case
        if chunks == 2:
            assert rows % (Ho * Wo) != 0 and rows % Wo != 0 and (M - rows) % 8 != 0, case
    B, H, W = WGRAD_CASES["m297_two_chunks_36x68"][:3]
    assert B * H * W == 297 and _wgrad_rows_per_chunk(297, 36, 68, 9) == 256 and 256 // 99 == 2 and (256 % 99) // 11 == 5 and 256 % 11 == 3
