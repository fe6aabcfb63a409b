"""The operators SurfaceNormalDORN's scene-understanding module needs under autograd (vi_depth_completion_amd/torch_ops.py): the dilated
conv, the average pool and the head with up to four output channels and pad 0 -- registration and shape functions on the CPU; on the GPU
every new kernel alone at the smallest shapes that reach its branches, then one composition shaped like SceneUnderstandingModuleBN.

The bars are made as tests/test_torch_ops_autograd.py describes in its header, by that file's own `_compare`: the float64 stock-PyTorch
restatement is differentiated by torch, the same restatement in float32 on the CPU gives the deviation, times 4 is what the fp32 kernels
get; precision 1 gets the ratio tests/test_torch_ops.py grants the direct bf16x3 form over fp32 (both are held to 2e-4 there: 1).  The ReLU
gates use the same `delta` rule (5 x the forward tolerance of tests/test_torch_ops.py: 1e-3 for a conv, 1e-4 for the head) with its 1 %
cap; `test_relu_gates_stay_under_the_cap` checks on the CPU that the float64 side of every gated case stays under it.  Pure data movement
(the operand writer, uncovered pool rows, dilation 1 against the plain entries) is compared bit for bit.
"""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402
from test_torch_ops_autograd import _compare, _nchw, _nhwc  # noqa: E402  (the harness that file's header describes)

from vi_depth_completion_amd import synthetic as S  # noqa: E402
from vi_depth_completion_amd import torch_ops as T  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
V = torch.ops.vidc
CONV_DELTA, HEAD_DELTA = 1e-3, 1e-4

# (H, W, Cin, dilation, pad): most taps outside the image; dense overlap; pad != dilation (output 5x7, M = 70); DORN's own geometry
DILATED_CASES = [(7, 9, 64, 6, 6), (5, 6, 64, 2, 2), (9, 11, 64, 3, 1), (30, 40, 128, 18, 18)]
# (H, W, kernel, stride, padding): DORN's own pooling; overlapping windows; rows and columns 8-9 in no window
POOL_CASES = [(30, 40, (8, 8), (8, 8), (1, 0)), (7, 9, (3, 3), (2, 2), (1, 1)), (10, 10, (4, 4), (4, 4), (0, 0))]
HEAD_CASES = [(0, False), (0, True), (1, False), (1, True)]       # (pad, relu), three output channels


def _ids(cases):
    return ["-".join(str(v).replace(" ", "") for v in c) for c in cases]


def _dilated_case(H, W, cin, d, pad, cout=32):
    seed = 100 * d + pad
    x = S.normal01(seed, "dorn.x", (2, cin, H, W)).float()
    w = S.normal01(seed, "dorn.w", (cout, cin, 3, 3)).float() * (2.0 / (cin * 9)) ** 0.5
    scale = 0.5 + S.uniform01(seed, "dorn.s", (cout,)).float()
    shift = 0.1 * S.normal01(seed, "dorn.b", (cout,)).float()
    return x, w, scale, shift


def _dilated_ref(d, pad, relu=True):
    def ref(x, w, scale, shift):
        pre = F.conv2d(x, w, padding=pad, dilation=d) * scale[None, :, None, None] + shift[None, :, None, None]
        return (F.relu(pre) if relu else pre), pre
    return ref


def _head_case():
    x = S.normal01(21, "dorn.hx", (2, 64, 6, 8)).float()
    w = S.normal01(21, "dorn.hw", (3, 64, 1, 1)).float() * 0.1
    b = torch.tensor([0.3, -0.2, 0.1])
    return x, w, b


def _head_ref(pad, relu):
    def ref(x, w, b):
        pre = F.interpolate(F.conv2d(x, w, b, padding=pad), size=(24, 32), mode="bilinear", align_corners=True)
        return (F.relu(pre) if relu else pre), pre
    return ref


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_dorn_ops_are_registered():
    assert len(T.BACKWARD_OPS) == 7
    assert set(T.DORN_BACKWARD_OPS) == {"conv2d_dilated_bn_act_backward", "avgpool2d_backward"}
    for name in ("conv2d_dilated_bn_act", "avgpool2d") + tuple(T.DORN_BACKWARD_OPS):
        assert hasattr(V, name), name
        assert name in T.OPS, name
        assert name not in T.BACKWARD_OPS
    assert len(set(T.OPS)) == len(T.OPS)


def test_dorn_shape_functions():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w, s = torch.empty(2, 30, 40, 128), torch.empty(64, 128, 3, 3), torch.empty(64)
        for precision in (0, 1, 2, 3):
            y = V.conv2d_dilated_bn_act(x, w, s, s, 18, 18, True, precision)
            assert y.shape == (2, 30, 40, 64) and y.dtype == torch.float32
        assert V.conv2d_dilated_bn_act(x, w, s, s, 1, 3, False, 0).shape == (2, 26, 36, 64)
        dy = torch.empty(2, 26, 36, 64)
        dx, dw, ds, db = V.conv2d_dilated_bn_act_backward(dy, x, w, dy, s, s, 30, 40, 1, 3, True, 0, True, True, True, False)
        assert dx.shape == x.shape and dw.shape == w.shape and ds.shape == s.shape and db.shape == s.shape
        assert {t.dtype for t in (dx, dw, ds, db)} == {torch.float32}
        dx, dw, ds, db = V.conv2d_dilated_bn_act_backward(dy, None, w, dy, s, s, 30, 40, 1, 3, True, 0, True, False, False, False)     # a frozen weight
        assert dx.shape == x.shape and dw.numel() == 0 and ds.numel() == 0 and db.numel() == 0
        dx, dw, ds, db = V.conv2d_dilated_bn_act_backward(dy, x, w, dy, s, s, 30, 40, 1, 3, True, 0, False, True, False, False)        # a frozen input
        assert dx.numel() == 0 and dw.shape == w.shape
        p = V.avgpool2d(x, 8, 8, 8, 8, 1, 0)
        assert p.shape == (2, 4, 5, 128) and p.dtype == torch.float32
        assert V.avgpool2d(torch.empty(2, 7, 9, 64), 3, 3, 2, 2, 1, 1).shape == (2, 4, 5, 64)
        assert V.avgpool2d(torch.empty(2, 10, 10, 64), 4, 4, 4, 4, 0, 0).shape == (2, 2, 2, 64)
        assert V.avgpool2d_backward(p, 30, 40, 8, 8, 8, 8, 1, 0).shape == x.shape
        hw = torch.empty(3, 128, 1, 1)
        assert V.head_conv1x1_upsample(x, hw, torch.empty(3), 0, 240, 320, False).shape == (2, 3, 240, 320)
        dx, dw, db = V.head_conv1x1_upsample_backward(torch.empty(2, 3, 240, 320), x, hw, None, 0)
        assert dx.shape == x.shape and dw.shape == hw.shape and db.shape == (3,)


def test_dorn_ops_carry_a_backward_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(), torch.enable_grad():
        x = torch.empty(2, 30, 40, 128, requires_grad=True)
        w = torch.empty(64, 128, 3, 3, requires_grad=True)
        s, b = torch.empty(64, requires_grad=True), torch.empty(64, requires_grad=True)
        for precision in (0, 1):
            y = V.conv2d_dilated_bn_act(x, w, s, b, 6, 6, True, precision)
            assert y.requires_grad and y.grad_fn is not None
            gx, gw, gs, gb = torch.autograd.grad(y.sum(), (x, w, s, b))
            assert gx.shape == x.shape and gw.shape == w.shape and gs.shape == s.shape and gb.shape == b.shape
        assert torch.autograd.grad(V.conv2d_dilated_bn_act(x, w.detach(), s.detach(), b.detach(), 6, 6, True, 0).sum(), (x,))[0].shape == x.shape
        for precision, word in ((2, "plain bf16"), (3, "MXFP8")):
            with pytest.raises(RuntimeError, match=word):
                V.conv2d_dilated_bn_act(x, w, s, b, 6, 6, True, precision)
        p = V.avgpool2d(x, 8, 8, 8, 8, 1, 0)
        assert p.grad_fn is not None and torch.autograd.grad(p.sum(), (x,))[0].shape == x.shape
        hw, hb = torch.empty(3, 128, 1, 1, requires_grad=True), torch.empty(3, requires_grad=True)
        y = V.head_conv1x1_upsample(x, hw, hb, 0, 240, 320, False)
        gx, gw, gb = torch.autograd.grad(y.sum(), (x, hw, hb))
        assert gx.shape == x.shape and gw.shape == hw.shape and gb.shape == hb.shape
        with pytest.raises(RuntimeError, match="1 to 4 output channels"):
            V.head_conv1x1_upsample(x, torch.empty(5, 128, 1, 1, requires_grad=True), torch.empty(5), 0, 240, 320, False)
        with torch.no_grad():
            assert not V.avgpool2d(x, 8, 8, 8, 8, 1, 0).requires_grad


def test_relu_gates_stay_under_the_cap():
    """The float64 side alone: the seeds of the gated GPU cases leave at most 1 % of the pre-activations within delta of zero."""
    for H, W, cin, d, pad in DILATED_CASES:
        pre = _dilated_ref(d, pad)(*[t.double() for t in _dilated_case(H, W, cin, d, pad)])[1]
        assert (pre.abs() < CONV_DELTA).double().mean().item() <= 0.01, (H, W, d, pad)
    for pad in (0, 1):
        pre = _head_ref(pad, True)(*[t.double() for t in _head_case()])[1]
        assert (pre.abs() < HEAD_DELTA).double().mean().item() <= 0.01, pad


# ---- GPU: the dilated conv ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("case", DILATED_CASES, ids=_ids(DILATED_CASES))
def test_dilated_conv_gradient(case, precision):
    """dx (the conv kernel on the data-gradient weights, dilated), dw (vidc_conv_wgrad_dilated), dscale, dshift against float64
    F.conv2d(dilation=d) autograd."""
    H, W, cin, d, pad = case
    ours = lambda x, w, s, b: _nchw(V.conv2d_dilated_bn_act(_nhwc(x), w, s, b, pad, d, True, precision))
    _compare("conv2d_dilated_bn_act[%dx%d,d=%d,pad=%d,p=%d]" % (H, W, d, pad, precision), _dilated_ref(d, pad), ours, _dilated_case(H, W, cin, d, pad),
             ["x", "w", "scale", "shift"], delta=CONV_DELTA, ratio=1.0)


@gpu
@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0)])
def test_dilation_one_gives_the_plain_entries_bits(k, pad):
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, H, W, ci, co = 2, 9, 11, 64, 32
    x = _nhwc(S.normal01(31, "dorn.one.x", (B, ci, H, W)).float()).to(DEV)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    dc = S.normal01(31, "dorn.one.dc", (B, Ho, Wo, co)).float().to(DEV)
    st = L.current_stream()
    assert lib.vidc_conv_wgrad_dilated_scratch_bytes(B, Ho, Wo, co, ci, k, k) == lib.vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, co, ci, k, k)
    sc = torch.empty(lib.vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, co, ci, k, k) + 256, dtype=torch.uint8, device=DEV)
    old, new = torch.zeros(co, ci, k, k, device=DEV), torch.ones(co, ci, k, k, device=DEV)
    L.check(lib.vidc_conv_wgrad(L.ptr(dc), L.ptr(x), L.ptr(old), B, H, W, ci, ci, Ho, Wo, co, co, k, k, 1, pad, L.ptr(sc), st), "wgrad")
    L.check(lib.vidc_conv_wgrad_dilated(L.ptr(dc), L.ptr(x), L.ptr(new), B, H, W, ci, ci, Ho, Wo, co, co, k, k, 1, pad, 1, L.ptr(sc), st), "wgrad dilated")
    assert old.abs().max() > 0 and torch.equal(old, new)
    # dilation 0, and an output size that belongs to another dilation, are refused
    assert lib.vidc_conv_wgrad_dilated(L.ptr(dc), L.ptr(x), L.ptr(new), B, H, W, ci, ci, Ho, Wo, co, co, k, k, 1, pad, 0, L.ptr(sc), st) == -2
    if k == 3:
        assert lib.vidc_conv_wgrad_dilated(L.ptr(dc), L.ptr(x), L.ptr(new), B, H, W, ci, ci, Ho, Wo, co, co, k, k, 1, pad, 2, L.ptr(sc), st) == -2
    # ... and the operator with dilation 1 is conv2d_bn_act with stride 1, gradient for gradient
    w = (S.normal01(31, "dorn.one.w", (co, ci, k, k)).float() * (2.0 / (ci * k * k)) ** 0.5).to(DEV)
    s, b = (0.5 + S.uniform01(31, "dorn.one.s", (co,)).float()).to(DEV), (0.1 * S.normal01(31, "dorn.one.b", (co,)).float()).to(DEV)
    with torch.enable_grad():
        grads = []
        for op in (lambda *a: V.conv2d_bn_act(*a, 1, pad, True, 0), lambda *a: V.conv2d_dilated_bn_act(*a, pad, 1, True, 0)):
            leaves = [t.clone().requires_grad_() for t in (x, w, s, b)]
            grads.append(torch.autograd.grad((op(*leaves) * dc).sum(), leaves))
    for g_old, g_new in zip(*grads):
        assert torch.equal(g_old, g_new)


@gpu
def test_dilated_conv_computes_only_what_is_asked():
    from vi_depth_completion_amd import ops
    H, W, cin, d, pad = DILATED_CASES[1]
    x, w, scale, shift = [t.to(DEV) for t in _dilated_case(H, W, cin, d, pad)]
    xh = _nhwc(x)
    dy = S.normal01(32, "dorn.only.dy", (2, H, W, 32)).float().to(DEV)
    launched = []
    real_w, real_x = ops.conv_backward_weight, ops.conv_backward_data
    ops.conv_backward_weight = lambda *a, **k: (launched.append("w"), real_w(*a, **k))[1]
    ops.conv_backward_data = lambda *a, **k: (launched.append("x"), real_x(*a, **k))[1]
    try:
        with torch.no_grad():
            assert not V.conv2d_dilated_bn_act(xh, w, scale, shift, pad, d, True, 0).requires_grad
        with torch.enable_grad():
            xa, wa = xh.clone().requires_grad_(), w.clone().requires_grad_()
            (V.conv2d_dilated_bn_act(xa, wa, scale, shift, pad, d, True, 0) * dy).sum().backward()
            assert sorted(launched) == ["w", "x"]
            del launched[:]
            xb, wb = xh.clone().requires_grad_(), w.clone()                       # a frozen weight
            (V.conv2d_dilated_bn_act(xb, wb, scale, shift, pad, d, True, 0) * dy).sum().backward()
            assert launched == ["x"] and wb.grad is None and torch.equal(xa.grad, xb.grad)
            del launched[:]
            xc, wc = xh.clone(), w.clone().requires_grad_()                       # a frozen input
            (V.conv2d_dilated_bn_act(xc, wc, scale, shift, pad, d, True, 0) * dy).sum().backward()
            assert launched == ["w"] and xc.grad is None and torch.equal(wa.grad, wc.grad)
            assert not V.conv2d_dilated_bn_act(xh, w, scale, shift, pad, d, True, 2).requires_grad      # (the plain-bf16 forward itself is fine)
            with pytest.raises(RuntimeError, match="has no backward"):
                V.conv2d_dilated_bn_act(xa, wa, scale, shift, pad, d, True, 2)
    finally:
        ops.conv_backward_weight, ops.conv_backward_data = real_w, real_x
    y = V.conv2d_dilated_bn_act(xh, w, scale, shift, pad, d, True, 0)
    dx, dw, ds, db = V.conv2d_dilated_bn_act_backward(dy, None, w, y, scale, shift, H, W, pad, d, True, 0, True, False, False, False)
    assert dx.shape == xh.shape and dw.numel() == 0 and ds.numel() == 0 and db.numel() == 0
    dx, dw, ds, db = V.conv2d_dilated_bn_act_backward(dy, xh, w, y, scale, shift, H, W, pad, d, True, 0, False, True, False, False)
    assert dx.numel() == 0 and dw.shape == w.shape
    with pytest.raises(RuntimeError, match="stride 1"):
        ops.conv_backward_data(dy, w, H, W, 2, pad, 0, dilation=d)


# ---- GPU: the operand writer of the weight-gradient GEMM -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H,W,C,d,pad", [(7, 9, 64, 6, 6), (5, 6, 64, 2, 2), (9, 11, 64, 3, 1), (30, 40, 128, 18, 18), (9, 11, 30, 3, 1)])
def test_im2col_transposed_dilated_operands(H, W, C, d, pad):
    """xt[(tap*C + c)][m] against F.unfold(dilation=d): exact for split 0; split 2 the bf16 bit patterns of tests/bf16_ref.py; split 1 the
    [32 x hi | 32 x lo] units of the same rounding (hi = rne(v), lo = rne(v - hi)); + 4 the same rows in channel-major order.  C = 30 takes
    the scalar kernel.  With dilation 1 the new entry writes the plain entry's bits in every format."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, k = 2, 3
    x = S.normal01(33, "dorn.im2col", (B, C, H, W)).float()
    xd = _nhwc(x).to(DEV)
    st = L.current_stream()

    def run(entry, dil, Ho, Wo, Mp, split, words):
        out = torch.full((k * k * C, words), float("nan"), device=DEV)
        args = (L.ptr(xd), L.ptr(out), B, H, W, C, C, Ho, Wo, k, k, 1, pad) + ((dil,) if entry == "vidc_im2col_transposed_dilated" else ()) + (Mp, split, st)
        L.check(getattr(lib, entry)(*args), entry)
        return out.cpu()

    Ho, Wo = H + 2 * pad - d * (k - 1), W + 2 * pad - d * (k - 1)
    M = B * Ho * Wo
    Mp, Mq = (M + 31) // 32 * 32, (M + 63) // 64 * 64
    cols = F.unfold(x, k, dilation=d, padding=pad)                          # (B, C*k*k, Ho*Wo), rows ordered (c, tap)
    tap_major = cols.view(B, C, k * k, Ho * Wo).permute(2, 1, 0, 3).reshape(k * k * C, M)
    chan_major = cols.permute(1, 0, 2).reshape(C * k * k, M)
    for want, order in ((tap_major, 0), (chan_major, 4)):
        w32, w64 = F.pad(want, (0, Mp - M)), F.pad(want, (0, Mq - M))
        assert torch.equal(run("vidc_im2col_transposed_dilated", d, Ho, Wo, Mp, order, Mp), w32)
        hi, lo = R.bits(w32), R.bits(w32 - R.rounded(w32))
        units = torch.cat((hi.view(-1, Mp // 32, 32), lo.view(-1, Mp // 32, 32)), dim=2).reshape(-1, 2 * Mp)
        got = run("vidc_im2col_transposed_dilated", d, Ho, Wo, Mp, 1 | order, Mp)
        assert torch.equal(got.view(torch.int16).to(torch.int32) & 0xFFFF, units)
        got = run("vidc_im2col_transposed_dilated", d, Ho, Wo, Mq, 2 | order, Mq // 2)
        assert torch.equal(got.view(torch.int16).to(torch.int32) & 0xFFFF, R.bits(w64))
    Ho1, Wo1 = H + 2 * pad - (k - 1), W + 2 * pad - (k - 1)
    M1 = B * Ho1 * Wo1
    Mq1 = (M1 + 63) // 64 * 64
    for split in (0, 1, 2, 4, 5, 6):
        words = Mq1 // 2 if split & 2 else Mq1
        old, new = run("vidc_im2col_transposed", 1, Ho1, Wo1, Mq1, split, words), run("vidc_im2col_transposed_dilated", 1, Ho1, Wo1, Mq1, split, words)
        assert torch.equal(old.view(torch.int32), new.view(torch.int32)), split
    assert lib.vidc_im2col_transposed_dilated(L.ptr(xd), L.ptr(xd), B, H, W, C, C, Ho, Wo, k, k, 1, pad, 0, Mp, 0, st) == -2


# ---- GPU: the average pool --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_avgpool_forward_and_gradient(case):
    from vi_depth_completion_amd import ops
    H, W, kernel, stride, padding = case
    x = S.normal01(34, "dorn.pool", (2, 64, H, W)).float()
    geom = kernel + stride + padding
    ref = lambda t: (F.avg_pool2d(t, kernel, stride, padding, count_include_pad=True), None)
    y64, y32 = ref(x.double())[0], ref(x)[0].double()
    ours = _nchw(V.avgpool2d(_nhwc(x).to(DEV), *geom)).double().cpu()
    assert ours.shape == y64.shape
    scale = y64.abs().max().item()
    for kind, red in (("max", torch.max), ("mean", torch.mean)):
        ref_dev, our_dev = red((y32 - y64).abs()).item() / scale, red((ours - y64).abs()).item() / scale
        print("AVGPOOL forward %s %-4s f32-CPU %.3e  bar %.3e  ours %.3e" % (case, kind, ref_dev, 4 * ref_dev, our_dev))
        assert our_dev <= 4 * ref_dev, (kind, our_dev, 4 * ref_dev)
    _compare("avgpool2d[%dx%d,k%d,s%d]" % (H, W, kernel[0], stride[0]), ref, lambda t: _nchw(V.avgpool2d(_nhwc(t), *geom)), [x], ["x"])
    # run to run, and on a second stream: the same bits; pixels no window covers: exactly 0
    Ho, Wo = y64.shape[2:]
    dy = S.normal01(34, "dorn.pool.dy", (2, Ho, Wo, 64)).float().to(DEV)
    first, second = ops.avgpool2d_backward(dy, (H, W), kernel, stride, padding), ops.avgpool2d_backward(dy, (H, W), kernel, stride, padding)
    assert first.abs().max() > 0 and torch.equal(first, second)
    covered_h, covered_w = (Ho - 1) * stride[0] - padding[0] + kernel[0], (Wo - 1) * stride[1] - padding[1] + kernel[1]
    if covered_h < H or covered_w < W:
        assert covered_h == 8 and covered_w == 8
        assert not first[:, covered_h:].any() and not first[:, :, covered_w:].any() and first[:, :covered_h, :covered_w].ne(0).all()
    else:
        assert case != POOL_CASES[2]


@gpu
def test_avgpool_backward_on_channel_slices():
    """The C ABI with row strides above C: dy is channels 8..71 of rows 80 wide, dx channels 4..67 of rows 96 wide; the same bits as the dense call,
    and nothing outside the slice is written."""
    from vi_depth_completion_amd import _lib as L, ops
    lib = L.lib()
    H, W, (kh, kw), (sh, sw), (ph, pw) = POOL_CASES[1]
    B, C, Ho, Wo = 2, 64, 4, 5
    dy = S.normal01(35, "dorn.pool.slice", (B, Ho, Wo, C)).float().to(DEV)
    dense = ops.avgpool2d_backward(dy, (H, W), (kh, kw), (sh, sw), (ph, pw))
    dy_wide = torch.full((B, Ho, Wo, 80), float("nan"), device=DEV)
    dy_wide[..., 8:72] = dy
    dx_wide = torch.full((B, H, W, 96), 7.0, device=DEV)
    L.check(lib.vidc_avgpool2d_backward(L.ptr(dy_wide[..., 8:]), L.ptr(dx_wide[..., 4:]), B, H, W, C, 96, kh, kw, sh, sw, ph, pw, 80, L.current_stream()), "avgpool bwd")
    assert torch.equal(dx_wide[..., 4:68], dense)
    assert bool((dx_wide[..., :4] == 7.0).all()) and bool((dx_wide[..., 68:] == 7.0).all())
    # rows that are no multiple of 4 floats wide, and a pointer off the 16-byte grid, are refused
    assert lib.vidc_avgpool2d_backward(L.ptr(dy_wide), L.ptr(dx_wide), B, H, W, C, 95, kh, kw, sh, sw, ph, pw, 80, L.current_stream()) == -2
    assert lib.vidc_avgpool2d_backward(L.ptr(dy_wide[..., 1:]), L.ptr(dx_wide), B, H, W, C, 96, kh, kw, sh, sw, ph, pw, 80, L.current_stream()) == -2


# ---- GPU: the head ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad,relu", HEAD_CASES)
def test_three_channel_head_gradient(pad, relu):
    ours = lambda t, wt, bt: V.head_conv1x1_upsample(_nhwc(t), wt, bt, pad, 24, 32, relu)
    _compare("head_conv1x1_upsample[co=3,pad=%d,relu=%d]" % (pad, relu), _head_ref(pad, relu), ours, _head_case(), ["x", "w", "bias"],
             delta=HEAD_DELTA if relu else None)


@gpu
@pytest.mark.parametrize("relu", [False, True])
def test_one_channel_head_backward_keeps_its_bits(relu):
    """Cout = 1, pad = 1 through ops.head_conv1x1_upsample_backward against the calls it made before it learned other heads: vidc_relu_backward,
    the upsample backward of the B planes, vidc_head_backward."""
    from vi_depth_completion_amd import _lib as L, ops
    lib = L.lib()
    B, h, w, C, H, W = 2, 6, 8, 64, 24, 32
    x = _nhwc(S.normal01(36, "dorn.h1.x", (B, C, h, w)).float()).to(DEV)
    wt = (S.normal01(36, "dorn.h1.w", (1, C, 1, 1)).float() * 0.1).to(DEV)
    dy = S.normal01(36, "dorn.h1.dy", (B, 1, H, W)).float().to(DEV)
    y = V.head_conv1x1_upsample(x, wt, torch.tensor([0.3], device=DEV), 1, H, W, relu) if relu else None
    dx, dw, db = ops.head_conv1x1_upsample_backward(dy, x, wt, 1, y)
    st = L.current_stream()
    g = ops.relu_backward(dy, y) if relu else dy
    g_low = torch.empty(B, h + 2, w + 2, device=DEV)
    L.check(lib.vidc_upsample_bilinear_ac_backward(L.ptr(g), L.ptr(g_low), B, h + 2, w + 2, 1, 1, 1, H, W, st), "upsample bwd")
    dx2, dw2, db2 = torch.empty_like(x), torch.empty_like(wt), torch.empty(1, device=DEV)
    sc = torch.empty(lib.vidc_head_backward_scratch_bytes(B, h, w, C) + 256, dtype=torch.uint8, device=DEV)
    L.check(lib.vidc_head_backward(L.ptr(g_low), L.ptr(x), L.ptr(wt.reshape(1, C).contiguous()), L.ptr(dx2), L.ptr(dw2), L.ptr(db2), B, h, w, C, C, C, L.ptr(sc), st),
            "head_backward")
    assert db.shape == (1,) and dw.shape == wt.shape and dx.abs().max() > 0
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)


# ---- GPU: the composition ---------------------------------------------------------------------------------------------------------------------
class _Folded(nn.Module):
    """Conv2d + eval-mode BatchNorm2d folded into (scale, shift) + ReLU: what conv2d_bn_act / conv2d_dilated_bn_act take."""

    def __init__(self, cin, cout, k, dilation):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=dilation * (k // 2), dilation=dilation, bias=False)
        self.scale, self.shift = nn.Parameter(torch.ones(cout)), nn.Parameter(torch.zeros(cout))

    def forward(self, x):
        return F.relu(self.conv(x) * self.scale[None, :, None, None] + self.shift[None, :, None, None])


class _Scene(nn.Module):
    """SceneUnderstandingModuleBN (surface_normal_dorn.py:37-79) at reduced size, without its Dropout2d layers: 64 input channels on a 6x8 map,
    32 per branch, AvgPool2d(2, 2) in the encoder, dilation 2 and 4, the three-channel head upsampled to 24x32."""

    def __init__(self, C=64, mid=32):
        super().__init__()
        self.pool, self.fc, self.enc = nn.AvgPool2d(2, stride=2), nn.Linear(C * 3 * 4, mid), nn.Conv2d(mid, mid, 1)
        self.aspp1, self.aspp2, self.aspp3 = _Folded(C, mid, 1, 1), _Folded(C, mid, 3, 2), _Folded(C, mid, 3, 4)
        self.cat, self.head = nn.Conv2d(4 * mid, 64, 1), nn.Conv2d(64, 3, 1)
        self.up_enc, self.up = nn.UpsamplingBilinear2d(size=(6, 8)), nn.UpsamplingBilinear2d(size=(24, 32))

    def forward(self, x):
        e = F.relu(self.fc(self.pool(x).flatten(1)))
        cat = torch.cat((self.up_enc(self.enc(e[:, :, None, None])), self.aspp1(x), self.aspp2(x), self.aspp3(x)), dim=1)
        return F.normalize(self.up(self.head(F.relu(self.cat(cat)))), dim=1)


_SCENE_NAMES = ["fc.weight", "fc.bias", "enc.weight", "enc.bias"] + [a + p for a in ("aspp1.", "aspp2.", "aspp3.") for p in ("conv.weight", "scale", "shift")] + \
    ["cat.weight", "cat.bias", "head.weight", "head.bias"]


def _scene_case():
    shapes = {n: tuple(p.shape) for n, p in _Scene().named_parameters()}
    assert sorted(shapes) == sorted(_SCENE_NAMES)
    wts = []
    for n in _SCENE_NAMES:
        shp = shapes[n]
        if n.endswith("scale"):
            wts.append(0.5 + S.uniform01(41, "scene." + n, shp).float())
        elif len(shp) == 1:
            wts.append(0.1 * S.normal01(41, "scene." + n, shp).float())
        else:
            wts.append(S.normal01(41, "scene." + n, shp).float() * (2.0 / (shp[1] * (shp[2] * shp[3] if len(shp) == 4 else 1))) ** 0.5)
    x = S.normal01(41, "scene.x", (1, 64, 6, 8)).float()
    mask = (S.uniform01(41, "scene.mask", (1, 1, 24, 32)) > 0.3).float()
    gt = F.normalize(S.normal01(41, "scene.gt", (1, 3, 24, 32)).float(), dim=1)
    return x, wts, mask, gt


def _scene_ref(mask, gt):
    net = _Scene()

    def ref(x, *wts):
        n = torch.func.functional_call(net, dict(zip(_SCENE_NAMES, wts)), (x,))
        return ((n - gt.to(x.dtype)).abs() * mask.to(x.dtype)).sum().reshape(1) / mask.sum().item(), None
    return ref


@gpu
def test_scene_understanding_composition_matches_float64_module():
    """avgpool2d -> flatten -> Linear (conv2d_bn_act on the (B, 1, 1, h*w*C) view, the weight permuted as engine.linear permutes it; its weight
    gradient is a one-row reduction, M = B = 1) -> ReLU -> 1x1 -> broadcast upsample | a 1x1 branch | two dilated branches -> torch.cat -> 1x1 +
    ReLU -> three-channel pad-0 head -> F.normalize -> masked L1 against unit normals: the gradient of every weight, scale, shift and of
    the input against the float64 torch.nn module."""
    x, wts, mask, gt = _scene_case()
    mask_d, gt_d = mask.to(DEV), gt.to(DEV)

    def ours(x_, fc_w, fc_b, enc_w, enc_b, w1, s1, b1, w2, s2, b2, w3, s3, b3, cat_w, cat_b, head_w, head_b):
        one = lambda t: torch.ones_like(t)
        xh = _nhwc(x_)
        e = V.avgpool2d(xh, 2, 2, 2, 2, 0, 0)                                                                    # (1, 3, 4, 64)
        fc = fc_w.view(-1, 64, 3, 4).permute(0, 2, 3, 1).reshape(-1, 3 * 4 * 64, 1, 1)                           # (c, h, w) -> (h, w, c) columns
        e = V.conv2d_bn_act(e.reshape(1, 1, 1, -1), fc, one(fc_b), fc_b, 1, 0, True, 0)
        e = V.upsample_bilinear_ac(V.conv2d_bn_act(e, enc_w, one(enc_b), enc_b, 1, 0, False, 0), 6, 8, False)     # from 1x1: a broadcast
        cat = torch.cat((e, V.conv2d_bn_act(xh, w1, s1, b1, 1, 0, True, 0), V.conv2d_dilated_bn_act(xh, w2, s2, b2, 2, 2, True, 0),
                         V.conv2d_dilated_bn_act(xh, w3, s3, b3, 4, 4, True, 0)), dim=3)
        h = V.conv2d_bn_act(cat, cat_w, one(cat_b), cat_b, 1, 0, True, 0)
        n = F.normalize(V.head_conv1x1_upsample(h, head_w, head_b, 0, 24, 32, False), dim=1)
        return ((n - gt_d).abs() * mask_d).sum().reshape(1) / mask.sum().item()

    _compare("scene", _scene_ref(mask, gt), ours, [x] + wts, ["x"] + _SCENE_NAMES, how="l1")
