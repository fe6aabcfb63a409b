"""Autograd of `torch.ops.vidc.*` (vi_depth_completion_amd/torch_ops.py): registration and shape functions of the backward operators on
the CPU; on the GPU the gradients against the same functions restated with stock PyTorch in float64 on the CPU.

How the bars are made (nothing is typed in by hand): the float64 restatement is differentiated by torch's own autograd; the identical
restatement is run in float32 on the CPU as well, and ITS max-abs / mean-abs deviation from the float64 gradients, normalised by the
float64 gradient's max-abs, times 4 is what our fp32 kernels get (precision 1: times the ratio tests/test_torch_ops.py grants that form
over fp32 -- 10 for Winograd, 1 for the direct form).  Every element of every gradient is compared.  ReLU gates: dy is set to zero, for
both sides, wherever the float64 pre-activation is within `delta` (5 x the forward tolerance of tests/test_torch_ops.py) of zero, and at
most 1 % of the positions may be zeroed that way.

Most test modules switch gradients off process-wide at import, so every gradient test runs inside `torch.enable_grad()`.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vidc_oracle as O
from vi_depth_completion_amd import synthetic as S
from vi_depth_completion_amd import torch_ops as T

FX, FY, CX, CY = 202.0, 202.0, 159.93827, 119.938015
V = torch.ops.vidc


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_ops_are_registered():
    assert len(T.BACKWARD_OPS) == 7
    for name in T.BACKWARD_OPS:
        assert hasattr(V, name), name
        assert name in T.OPS, name
    assert "conv3x3_winograd" in T.OPS
    for name in ("warp2dof_fwd", "warp2dof_inv_rot_norm", "stem_conv3x3s2", "maxpool3x3s2", "upsample_bilinear_ac", "head_conv1x1_upsample",
                 "conv2d_bn_act"):
        assert name + "_backward" in T.BACKWARD_OPS


def test_backward_shape_functions():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img, g = torch.empty(2, 3, 240, 320), torch.empty(2, 3)
        for ac in (False, True):
            dx = V.warp2dof_fwd_backward(img, g, g, FX, FY, CX, CY, ac)
            assert dx.shape == img.shape and dx.dtype == torch.float32
            for normalize in (False, True):
                assert V.warp2dof_inv_rot_norm_backward(img, img, g, g, FX, FY, CX, CY, ac, normalize).shape == img.shape
        x, w, s = torch.empty(2, 60, 80, 64), torch.empty(128, 64, 3, 3), torch.empty(128)
        for stride, dy in ((2, torch.empty(2, 30, 40, 128)), (1, torch.empty(2, 60, 80, 128))):
            dx, dw, ds, db = V.conv2d_bn_act_backward(dy, x, w, dy, s, s, 60, 80, stride, 1, True, 0, True, True, True, False)
            assert dx.shape == x.shape and dw.shape == w.shape and ds.shape == s.shape and db.shape == s.shape
            assert {t.dtype for t in (dx, dw, ds, db)} == {torch.float32}
        dx, dw, ds, db = V.conv2d_bn_act_backward(dy, None, w, dy, s, s, 60, 80, 1, 1, True, 1, True, False, False, False)      # a frozen weight
        assert dx.shape == x.shape and dw.numel() == 0 and ds.numel() == 0 and db.numel() == 0
        sx, sw = torch.empty(2, 3, 240, 320), torch.empty(64, 3, 3, 3)
        dx, dw = V.stem_conv3x3s2_backward(torch.empty(2, 120, 160, 64), sx, sw, torch.empty(2, 120, 160, 64), 240, 320, True, True, True)
        assert dx.shape == sx.shape and dw.shape == sw.shape
        assert V.maxpool3x3s2_backward(torch.empty(2, 30, 40, 64), x).shape == x.shape
        assert V.upsample_bilinear_ac_backward(torch.empty(2, 120, 160, 64), None, 60, 80).shape == x.shape
        assert V.upsample_bilinear_ac_backward(torch.empty(2, 120, 160, 64), torch.empty(2, 120, 160, 64), 60, 80).shape == x.shape
        hw = torch.empty(1, 64, 1, 1)
        dx, dw, db = V.head_conv1x1_upsample_backward(torch.empty(2, 1, 240, 320), x, hw, torch.empty(2, 1, 240, 320), 1)
        assert dx.shape == x.shape and dw.shape == hw.shape and db.shape == (1,)


def test_forward_ops_carry_a_backward_under_fake_tensors():
    """The registration itself, without a GPU: an output of a differentiable operator has a grad_fn, and the backward graph runs through the
    backward operators' shape functions."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(), torch.enable_grad():
        x = torch.empty(2, 60, 80, 64, requires_grad=True)
        w = torch.empty(128, 64, 3, 3, requires_grad=True)
        s, b = torch.empty(128, requires_grad=True), torch.empty(128, requires_grad=True)
        y = V.conv2d_bn_act(x, w, s, b, 2, 1, True, 0)
        assert y.requires_grad and y.grad_fn is not None
        gx, gw, gs, gb = torch.autograd.grad(y.sum(), (x, w, s, b))
        assert gx.shape == x.shape and gw.shape == w.shape and gs.shape == s.shape and gb.shape == b.shape
        y = V.conv3x3_winograd(x, w, s, b, 4, True, 1)
        assert torch.autograd.grad(y.sum(), (x,))[0].shape == x.shape
        with pytest.raises(RuntimeError, match="MXFP8"):
            V.conv2d_bn_act(x, w, s, b, 2, 1, True, 3)
        img = torch.empty(2, 3, 240, 320, requires_grad=True)
        g = torch.empty(2, 3)
        _h, z = V.warp2dof_inv_rot_norm(img, g, g, FX, FY, CX, CY, False, True)
        assert torch.autograd.grad(z.sum(), (img,))[0].shape == img.shape
        with pytest.raises(RuntimeError, match="not differentiable"):
            V.warp2dof_fwd(img, g.clone().requires_grad_(), g, FX, FY, CX, CY, False)
        with torch.no_grad():
            assert not V.maxpool3x3s2(x).requires_grad


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------------------------
def _grads(fn, tensors, dtype, dy, device="cpu"):
    leaves = [t.detach().to(dtype).to(device).requires_grad_() for t in tensors]
    out = fn(*leaves)
    out = out[0] if isinstance(out, tuple) else out
    return [g.detach().double().cpu() for g in torch.autograd.grad((out * dy.to(dtype).to(device)).sum(), leaves)]


def _compare(name, ref_fn, our_fn, tensors, names, delta=None, ratio=1.0, how="elementwise"):
    """ref_fn(*leaves) -> (out, pre-activation or None) in any dtype on the CPU; our_fn(*leaves) -> out on the GPU, same layout."""
    failures = []
    with torch.enable_grad():
        out64, pre64 = ref_fn(*[t.double() for t in tensors])
        dy = S.normal01(77, name + ".dy", tuple(out64.shape)).double()
        if delta is not None:
            gate = pre64.abs() < delta
            frac = gate.double().mean().item()
            print("%s: dy zeroed at %.4f %% of the positions (|pre-activation| < %g)" % (name, 100 * frac, delta))
            assert frac <= 0.01, "badly chosen input: %.3f %% of the ReLU gates within delta" % (100 * frac)
            dy = dy.masked_fill(gate, 0.0)
        ref = lambda *a: ref_fn(*a)[0]
        g64 = _grads(ref, tensors, torch.float64, dy)
        g32 = _grads(ref, tensors, torch.float32, dy)
        ours = _grads(our_fn, tensors, torch.float32, dy, "cuda")
    for n, a, b, c in zip(names, g64, g32, ours):
        assert c.shape == a.shape, (n, c.shape, a.shape)
        if how == "elementwise":
            scale = a.abs().max().item()
            figs = [("max", (b - a).abs().max().item() / scale, (c - a).abs().max().item() / scale),
                    ("mean", (b - a).abs().mean().item() / scale, (c - a).abs().mean().item() / scale)]
        else:                     # the robust figure of a chain: sum |ours - f64| / sum |f64|; the max-abs deviation is printed only
            tot = a.abs().sum().item()
            figs = [("l1", (b - a).abs().sum().item() / tot, (c - a).abs().sum().item() / tot)]
            print("AUTOGRAD %-34s d%-6s max-abs deviation / max|f64|: f32-CPU %.3e ours %.3e (not asserted)"
                  % (name, n, (b - a).abs().max().item() / a.abs().max().item(), (c - a).abs().max().item() / a.abs().max().item()))
        for kind, ref_dev, our_dev in figs:
            bar = 4.0 * ratio * ref_dev
            ok = our_dev <= bar
            print("AUTOGRAD %-34s d%-6s %-4s f32-CPU %.3e  bar %.3e  ours %.3e  %s" % (name, n, kind, ref_dev, bar, our_dev, "ok" if ok else "MISS"))
            if not ok:
                failures.append((name, n, kind, our_dev, bar))
    assert not failures, failures


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _batch():
    b = S.synthetic_batch(2, 240, 320, 1234)
    return b["image"], b["gravity"], b["aligned_direction"], O.Intrinsics(FX, FY, CX, CY)


# ---- 1. reference gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("align_corners", [False, True])
def test_warp_fwd_gradient(align_corners):
    img, g, a, intr = _batch()
    _, _, grid = O.forward_grid(g, a, intr)
    ref = lambda x: (F.grid_sample(x, grid.to(x.dtype), mode="bilinear", padding_mode="zeros", align_corners=align_corners), None)
    ours = lambda x: V.warp2dof_fwd(x, g.cuda(), a.cuda(), FX, FY, CX, CY, align_corners)[1]
    _compare("warp2dof_fwd[ac=%d]" % align_corners, ref, ours, [img], ["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("align_corners", [False, True])
def test_warp_inv_rot_norm_gradient(align_corners, normalize):
    _img, g, a, intr = _batch()
    nmap = S.normal01(1234, "ops.normalmap", (2, 3, 240, 320)).float()
    _, R, grid = O.inverse_grid(g, a, intr)

    def ref(x):
        y = F.grid_sample(x, grid.to(x.dtype), mode="bilinear", padding_mode="zeros", align_corners=align_corners)
        z = R.to(x.dtype).permute(0, 2, 1).bmm(y.view(2, 3, -1)).view(2, 3, 240, 320)
        return (F.normalize(z, dim=1) if normalize else z), None

    ours = lambda x: V.warp2dof_inv_rot_norm(x, g.cuda(), a.cuda(), FX, FY, CX, CY, align_corners, normalize)[1]
    _compare("warp2dof_inv_rot_norm[ac=%d,n=%d]" % (align_corners, normalize), ref, ours, [nmap], ["x"])


def _conv_case(seed, shape_x):
    x = S.normal01(seed, "ops.x", shape_x).float()
    w = S.normal01(seed, "ops.w", (96, 64, 3, 3)).float() * (2.0 / (64 * 9)) ** 0.5
    scale = 0.5 + S.uniform01(seed, "ops.s", (96,)).float()
    shift = 0.1 * S.normal01(seed, "ops.b", (96,)).float()
    return x, w, scale, shift


def _conv_ref(stride, relu):
    def ref(x, w, scale, shift):
        pre = F.conv2d(x, w, stride=stride, padding=1) * scale[None, :, None, None] + shift[None, :, None, None]
        return (F.relu(pre) if relu else pre), pre
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_gradient(stride, relu, precision):
    """The direct form at precision 1 is granted no more than fp32 (ratio 1), so its data gradient runs in exact fp32: in the forward's
    split-bf16 arithmetic dx measured 3.9e-6..5.0e-6 max / 5.3e-7..7.7e-7 mean of max|dx| on MI355X against bars of 0.83e-6..3.3e-6 /
    0.91e-7..1.5e-7 (profiles/EXPERIMENTS.md)."""
    tensors = _conv_case(7, (2, 64, 30, 40))
    ours = lambda x, w, s, b: _nchw(V.conv2d_bn_act(_nhwc(x), w, s, b, stride, 1, relu, precision))
    _compare("conv2d_bn_act[s=%d,relu=%d,p=%d]" % (stride, relu, precision), _conv_ref(stride, relu), ours, tensors, ["x", "w", "scale", "shift"],
             delta=1e-3 if relu else None, ratio=1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("m", [2, 4])
def test_winograd_conv_gradient(m, precision):
    tensors = _conv_case(8, (2, 64, 30, 41))
    ours = lambda x, w, s, b: _nchw(V.conv3x3_winograd(_nhwc(x), w, s, b, m, True, precision))
    _compare("conv3x3_winograd[m=%d,p=%d]" % (m, precision), _conv_ref(1, True), ours, tensors, ["x", "w", "scale", "shift"],
             delta=1e-2 if precision == 1 else 1e-3, ratio=10.0 if precision == 1 else 1.0)


@pytest.mark.gpu
def test_glue_gradients():
    x = S.normal01(9, "ops.g", (2, 64, 31, 41)).float()
    _compare("maxpool3x3s2", lambda t: (F.max_pool2d(t, 3, 2, 1), None), lambda t: _nchw(V.maxpool3x3s2(_nhwc(t))), [x], ["x"])
    for relu in (False, True):
        def ref(t):
            pre = F.interpolate(t, size=(62, 82), mode="bilinear", align_corners=True)
            return (F.relu(pre) if relu else pre), pre
        _compare("upsample_bilinear_ac[relu=%d]" % relu, ref, lambda t: _nchw(V.upsample_bilinear_ac(_nhwc(t), 62, 82, relu)), [x], ["x"],
                 delta=5e-5 if relu else None)
    img = S.uniform01(9, "ops.img", (2, 3, 240, 320)).float()
    w = S.normal01(9, "ops.sw", (64, 3, 3, 3)).float() * 0.2

    def stem_ref(t, wt):
        pre = F.conv2d(t, wt, stride=2, padding=1)
        return F.relu(pre), pre
    _compare("stem_conv3x3s2", stem_ref, lambda t, wt: _nchw(V.stem_conv3x3s2(t, wt, True)), [img, w], ["x", "w"], delta=5e-5)
    hw = S.normal01(9, "ops.hw", (1, 64, 1, 1)).float() * 0.1
    hb = torch.tensor([0.3])

    def head_ref(t, wt, bt):
        pre = F.interpolate(F.conv2d(t, wt, bt, padding=1), size=(120, 160), mode="bilinear", align_corners=True)
        return F.relu(pre), pre
    _compare("head_conv1x1_upsample", head_ref, lambda t, wt, bt: V.head_conv1x1_upsample(_nhwc(t), wt, bt, 1, 120, 160, True), [x, hw, hb],
             ["x", "w", "bias"], delta=1e-4)


# ---- 2. transpose identity ----------------------------------------------------------------------------------------------------------------
def _identity_gap(fn, x, dy, dtype, device):
    """|<dy, op(x)> - <op^T(dy), x>| / sum |dy . op(x)|, both inner products accumulated in float64 on the host."""
    with torch.enable_grad():
        leaf = x.to(dtype).to(device).requires_grad_()
        out = fn(leaf)
        gx, = torch.autograd.grad((out * dy.to(dtype).to(device)).sum(), leaf)
    terms = out.detach().double().cpu() * dy.double()
    lhs, rhs = terms.sum().item(), (gx.double().cpu() * x.double()).sum().item()
    return abs(lhs - rhs) / terms.abs().sum().item()


@pytest.mark.gpu
def test_linear_operators_are_transposed_exactly():
    img, g, a, intr = _batch()
    nmap = S.normal01(1234, "ops.normalmap", (2, 3, 240, 320)).float()
    xg = S.normal01(9, "ops.g", (2, 64, 31, 41)).float()
    misses = []
    for ac in (False, True):
        _, _, fgrid = O.forward_grid(g, a, intr)
        _, R, igrid = O.inverse_grid(g, a, intr)
        cases = [
            ("warp2dof_fwd[ac=%d]" % ac, img, lambda x: F.grid_sample(x, fgrid, mode="bilinear", padding_mode="zeros", align_corners=ac),
             lambda x: V.warp2dof_fwd(x, g.cuda(), a.cuda(), FX, FY, CX, CY, ac)[1]),
            ("warp2dof_inv_rot_norm[ac=%d,n=0]" % ac, nmap,
             lambda x: R.permute(0, 2, 1).bmm(F.grid_sample(x, igrid, mode="bilinear", padding_mode="zeros", align_corners=ac).view(2, 3, -1)).view(2, 3, 240, 320),
             lambda x: V.warp2dof_inv_rot_norm(x, g.cuda(), a.cuda(), FX, FY, CX, CY, ac, False)[1]),
        ]
        if not ac:
            cases.append(("upsample_bilinear_ac", xg, lambda x: F.interpolate(x, size=(62, 82), mode="bilinear", align_corners=True),
                          lambda x: _nchw(V.upsample_bilinear_ac(_nhwc(x), 62, 82, False))))
        for name, x, ref, ours in cases:
            dy = S.normal01(78, name + ".dy", tuple(ref(x).shape)).float()
            ref_gap, our_gap = _identity_gap(ref, x, dy, torch.float32, "cpu"), _identity_gap(ours, x, dy, torch.float32, "cuda")
            ok = our_gap <= 4 * ref_gap
            print("TRANSPOSE %-34s f32-CPU %.3e  bar %.3e  ours %.3e  %s" % (name, ref_gap, 4 * ref_gap, our_gap, "ok" if ok else "MISS"))
            if not ok:
                misses.append((name, our_gap, 4 * ref_gap))
    assert not misses, misses


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_new_backward_kernels_are_bit_reproducible():
    from vi_depth_completion_amd import ops
    from vi_depth_completion_amd.networks.warping_2dof_alignment import Warping2DOFAlignment
    img, g, a, _intr = _batch()
    wp = Warping2DOFAlignment(FX, FY, CX, CY, device="cuda")
    params = wp._params(g.cuda(), a.cuda())
    dy = S.normal01(79, "det.dy", (2, 3, 240, 320)).float().cuda()
    nmap = S.normal01(1234, "ops.normalmap", (2, 3, 240, 320)).float().cuda()
    y = S.normal01(79, "det.y", (2, 15, 20, 96)).float().cuda().relu()
    gy = S.normal01(79, "det.gy", (2, 15, 20, 96)).float().cuda()
    scale, shift = (0.5 + S.uniform01(79, "det.s", (96,)).float()).cuda(), (0.1 * S.normal01(79, "det.b", (96,)).float()).cuda()
    sy = S.normal01(79, "det.sy", (2, 120, 160, 64)).float().cuda().relu()
    sg = S.normal01(79, "det.sg", (2, 120, 160, 64)).float().cuda()
    sw = (S.normal01(9, "ops.sw", (64, 3, 3, 3)).float() * 0.2).cuda()
    kernels = {
        "warp2dof_fwd_backward": lambda: (ops.warp2dof_fwd_backward(dy, params, CX, CY, False),),
        "warp2dof_inv_rot_norm_backward": lambda: (ops.warp2dof_inv_rot_norm_backward(nmap, dy, params, CX, CY, False, True),),
        "affine_act_backward": lambda: ops.affine_act_backward(gy, y, scale, shift, True),
        "stem_conv3x3s2_backward_data": lambda: (ops.stem_conv3x3s2_backward_data(sg, sy, sw, 240, 320, True),),
    }
    side = torch.cuda.Stream()
    for name, run in kernels.items():
        first, second = run(), run()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = run()
        side.synchronize()
        for p, q, r in zip(first, second, third):
            assert torch.isfinite(p).all() and p.abs().max() > 0, name
            assert torch.equal(p, q) and torch.equal(p, r), name


# ---- 4. only what is asked ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_only_requested_gradients_are_computed():
    x, w, scale, shift = [t.cuda() for t in _conv_case(7, (2, 64, 30, 40))]
    xh = _nhwc(x)
    with torch.no_grad():
        assert not V.conv2d_bn_act(xh, w, scale, shift, 2, 1, True, 0).requires_grad
        assert not V.warp2dof_fwd(torch.zeros(1, 3, 240, 320, device="cuda"), torch.tensor([[0.0, 1.0, 0.0]]).cuda(),
                                  torch.tensor([[0.0, 1.0, 0.0]]).cuda(), FX, FY, CX, CY, False)[1].requires_grad
    with torch.enable_grad():
        dy = S.normal01(80, "only.dy", (2, 15, 20, 96)).float().cuda()
        xa, wa = xh.clone().requires_grad_(), w.clone().requires_grad_()
        (V.conv2d_bn_act(xa, wa, scale, shift, 2, 1, True, 0) * dy).sum().backward()
        xb, wb = xh.clone().requires_grad_(), w.clone()
        launched = []
        from vi_depth_completion_amd import ops
        real = ops.conv_backward_weight
        ops.conv_backward_weight = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
        try:
            (V.conv2d_bn_act(xb, wb, scale, shift, 2, 1, True, 0) * dy).sum().backward()
        finally:
            ops.conv_backward_weight = real
        assert not launched and wb.grad is None and wa.grad is not None
        assert torch.equal(xa.grad, xb.grad)
        xm = S.normal01(80, "only.xm", (1, 8, 8, 128)).float().cuda()
        wm = (S.normal01(80, "only.wm", (64, 128, 3, 3)).float() * 0.03).cuda()
        one = torch.ones(64, device="cuda")
        assert not V.conv2d_bn_act(xm, wm, one, one, 1, 1, True, 3).requires_grad      # (the MXFP8 forward itself is fine)
        with pytest.raises(RuntimeError, match="MXFP8"):
            V.conv2d_bn_act(xm.clone().requires_grad_(), wm, one, one, 1, 1, True, 3)
        img = torch.zeros(1, 3, 240, 320, device="cuda", requires_grad=True)
        grav = torch.tensor([[0.0, 1.0, 0.0]]).cuda()
        with pytest.raises(RuntimeError, match="not differentiable"):
            V.warp2dof_fwd(img, grav.clone().requires_grad_(), grav, FX, FY, CX, CY, False)
        with pytest.raises(RuntimeError, match="not differentiable"):
            V.warp2dof_inv_rot_norm(img, grav, grav.clone().requires_grad_(), FX, FY, CX, CY, False, True)


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_of_operators_matches_float64_chain():
    img, g, a, intr = _batch()
    _, _, grid = O.forward_grid(g, a, intr)
    n = lambda name, shape, k: S.normal01(11, "chain." + name, shape).float() * k
    w_stem = n("ws", (64, 3, 3, 3), 0.2)
    w3, s3, b3 = n("w3", (64, 64, 3, 3), (2.0 / 576) ** 0.5), 0.5 + S.uniform01(11, "chain.s3", (64,)).float(), n("b3", (64,), 0.1)
    w1, s1, b1 = n("w1", (64, 64, 1, 1), (2.0 / 64) ** 0.5), 0.5 + S.uniform01(11, "chain.s1", (64,)).float(), n("b1", (64,), 0.1)
    wh, bh = n("wh", (1, 64, 1, 1), 0.1), torch.tensor([0.3])
    aff = lambda t, s, b: t * s[None, :, None, None] + b[None, :, None, None]

    def ref(x, ws, w3_, s3_, b3_, w1_, s1_, b1_, wh_, bh_):
        t = F.grid_sample(x, grid.to(x.dtype), mode="bilinear", padding_mode="zeros", align_corners=False)
        t = F.max_pool2d(F.relu(F.conv2d(t, ws, stride=2, padding=1)), 3, 2, 1)
        t = F.relu(aff(F.conv2d(t, w3_, padding=1), s3_, b3_))
        t = F.relu(aff(F.conv2d(t, w1_), s1_, b1_))
        t = F.interpolate(t, size=(120, 160), mode="bilinear", align_corners=True)
        return F.relu(F.interpolate(F.conv2d(t, wh_, bh_, padding=1), size=(240, 320), mode="bilinear", align_corners=True)), None

    def ours(x, ws, w3_, s3_, b3_, w1_, s1_, b1_, wh_, bh_):
        t = V.warp2dof_fwd(x, g.cuda(), a.cuda(), FX, FY, CX, CY, False)[1]
        t = V.maxpool3x3s2(V.stem_conv3x3s2(t, ws, True))
        t = V.conv3x3_winograd(t, w3_, s3_, b3_, 4, True, 0)
        t = V.conv2d_bn_act(t, w1_, s1_, b1_, 1, 0, True, 0)
        t = V.upsample_bilinear_ac(t, 120, 160, False)
        return V.head_conv1x1_upsample(t, wh_, bh_, 1, 240, 320, True)

    _compare("chain", ref, ours, [img, w_stem, w3, s3, b3, w1, s1, b1, wh, bh],
             ["image", "w_stem", "w3", "scale3", "shift3", "w1", "scale1", "shift1", "w_head", "b_head"], how="l1")
