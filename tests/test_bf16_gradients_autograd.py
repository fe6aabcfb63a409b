"""Plain-bf16 conv gradients under autograd: the `torch_ops.grad_precision` knob, ops.conv_backward_data / conv_backward_weight at precision 2,
the two conv backward operators inside the context, and SurfaceNormalPrediction.forward_autograd(grad_precision=2).

The rounding is part of the contract, so the references are the float64 restatements of tests/test_conv_backward_kernels.py on the ROUNDED
operands (R.rounded = bf16 round to nearest even): dx against ref_dgrad(q(dc), q(w)) under (K + 2) u S|q(dc) q(w)|, K = Cout x taps (that file's
precision-0 factor: the bf16 products are exact in fp32, one fp32 chain of K terms); dw against ref_wgrad(q(dc), q(x)) under
(n + 2) u S|q(dc) q(x)| (tests/test_wgrad_bf16_kernel.py).  In the operator tests `scale` holds exact powers of two and relu is off (or the
mask is taken from the operator's own forward output), so dc = mask(dy) * scale is known exactly and its rounding reproducible.
The network bars are those of tests/test_training.py::test_plain_bf16_training_mode, the project's own for bf16 training (a mode that also
rounds the forward, which is strictly weaker arithmetic): gradient cosine > 0.99, global gradient norm within 2e-2, six Adam steps bring the
loss under 0.9 x its start and within 5 % of the same steps with fp32 gradients.
"""
import inspect
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402
from test_conv_backward_kernels import (DGRAD_B, DGRAD_CASES, DGRAD_CIN, DGRAD_COUT, U, _dgrad_data, _out_size, _randn, _same_bits,  # noqa: E402
                                        _within, ref_dgrad, ref_wgrad)
from test_dorn_ops_autograd import DILATED_CASES  # noqa: E402
from test_sn_training import SMALL, _inputs, _network  # noqa: E402
from test_torch_ops_autograd import _nchw, _nhwc  # noqa: E402
from test_wgrad_bf16_kernel import _rows_per_chunk, ref_wgrad_dilated  # noqa: E402

from vi_depth_completion_amd import torch_ops as T  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
V = torch.ops.vidc
F64 = torch.float64


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_grad_precision_context_nests_restores_and_refuses():
    assert T.current_grad_precision() == 0
    with T.grad_precision(2):
        assert T.current_grad_precision() == 2
        with T.grad_precision(0):
            assert T.current_grad_precision() == 0
            with T.grad_precision(2):
                assert T.current_grad_precision() == 2
            assert T.current_grad_precision() == 0
        assert T.current_grad_precision() == 2
        for bad in (1, 3):
            with pytest.raises(RuntimeError, match="0 .*2"):
                with T.grad_precision(bad):
                    pass
        assert T.current_grad_precision() == 2
        with pytest.raises(KeyError):                 # an exception inside restores as well
            with T.grad_precision(0):
                raise KeyError("x")
        assert T.current_grad_precision() == 2
    assert T.current_grad_precision() == 0


def test_forward_autograd_signatures_and_begin_refuses_before_touching_the_module():
    from vi_depth_completion_amd.networks import autograd_blocks
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.networks.surface_normal_dorn import SurfaceNormalDORN
    for cls in (ModifiedFPN, SurfaceNormalPrediction, SurfaceNormalDORN):
        p = inspect.signature(cls.forward_autograd).parameters
        assert p["grad_precision"].default == 0 and p["precision"].default == 0, cls

    class Module(torch.nn.Module):
        pass

    class Cuda:                                       # (begin reads .is_cuda and .device of its tensors only)
        is_cuda, device = True, "cuda"
    m = Module().train()
    for bad in (1, 3):
        with pytest.raises(RuntimeError, match="grad_precision 0 .*2"):
            autograd_blocks.begin(m, (Cuda(),), 0, bad)
        assert not hasattr(m, "_autograd_dirty")
    with pytest.raises(RuntimeError, match="precision 0 .*1"):
        autograd_blocks.begin(m, (Cuda(),), 2, 2)                    # the forward's refusal stands
    walk = autograd_blocks.begin(m, (Cuda(),), 0, 2)
    assert m._autograd_dirty and T.current_grad_precision() == 0
    with walk.grads():
        assert T.current_grad_precision() == 2
    assert T.current_grad_precision() == 0


def test_backward_operators_at_precision_2_have_the_shapes_of_the_shape_function():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w, s = torch.empty(2, 9, 11, 64), torch.empty(64, 64, 3, 3), torch.empty(64)
        dy = torch.empty(2, 9, 11, 64)
        for need in ((True, True, True), (True, False, False), (False, True, False)):
            want = T._conv_backward_shapes(dy, w, s, s, 9, 11, *need)
            got = V.conv2d_bn_act_backward(dy, x, w, dy, s, s, 9, 11, 1, 1, True, 2, *need, False)
            assert [t.shape for t in got] == [t.shape for t in want] and {t.dtype for t in got} == {torch.float32}
            got = V.conv2d_dilated_bn_act_backward(dy, x, w, dy, s, s, 9, 11, 2, 2, True, 2, *need, False)
            assert [t.shape for t in got] == [t.shape for t in want] and {t.dtype for t in got} == {torch.float32}
        dy2 = torch.empty(2, 5, 6, 64)
        got = V.conv2d_bn_act_backward(dy2, x, w, dy2, s, s, 9, 11, 2, 1, False, 2, True, True, True, False)
        assert [t.shape for t in got] == [x.shape, w.shape, s.shape, s.shape]
    with FakeTensorMode(), torch.enable_grad():          # ... and through autograd, the forward inside the context
        leaves = [torch.empty(sh, requires_grad=True) for sh in ((2, 9, 11, 64), (64, 64, 3, 3), (64,), (64,))]
        with T.grad_precision(2):
            ys = [V.conv2d_bn_act(*leaves, 2, 1, True, 0), V.conv2d_dilated_bn_act(*leaves, 2, 2, True, 1), V.conv3x3_winograd(*leaves, 4, True, 1)]
        for y in ys:
            assert [g.shape for g in torch.autograd.grad(y.sum(), leaves)] == [t.shape for t in leaves]


def test_one_item_packer_refuses_without_a_device():
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    p = 4096
    assert lib.vidc_pack_conv_weights_one(None, p, 64, 32, 3, 3, 5, None) == -1 and lib.vidc_pack_conv_weights_one(p, None, 64, 32, 3, 3, 5, None) == -1
    for co, ci, k, kind in ((36, 32, 3, 5), (32, 32, 3, 5), (64, 32, 5, 5), (64, 32, 3, 6), (48, 32, 3, 3), (64, 0, 3, 5)):
        assert lib.vidc_pack_item_blocks(co, ci, k, k, kind) == 0 and lib.vidc_pack_conv_weights_one(p, p, co, ci, k, k, kind, None) == -2, (co, ci, k, kind)


# ---- GPU: wrappers -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", DGRAD_CASES, ids=["k%d_s%d_p%d_%dx%d" % c for c in DGRAD_CASES])
def test_conv_backward_data_bf16(case):
    """ops.conv_backward_data(..., precision=2) against ref_dgrad on the rounded operands under (K + 2) u S|q(dc) q(w)|; pixels no window covers
    are exactly 0."""
    from vi_depth_completion_amd import ops
    k, stride, pad, H, W = case
    dc, w = _dgrad_data(*case)
    assert ops.conv_backward_data_precision((DGRAD_COUT, DGRAD_CIN, k, k), 2) == 2
    want, mag = ref_dgrad(R.rounded(dc), R.rounded(w), H, W, stride, pad)
    got = ops.conv_backward_data(_nhwc(dc).to(DEV), w.to(DEV), H, W, stride, pad, 2)
    assert got.shape == (DGRAD_B, H, W, DGRAD_CIN) and got.is_contiguous() and got.dtype == torch.float32
    if k == 1 and stride == 2:
        assert float(mag[:, :, 1::2].max()) == 0.0 and not bool(_nchw(got.cpu())[:, :, 1::2].any())
    _within("dx_bf16", _nchw(got.cpu()), want, mag, DGRAD_COUT * k * k + 2, "%s precision 2" % (case,))
    print("\n[conv_backward_data bf16 %s] error / bound %.3f" % (case, __import__("test_conv_backward_kernels").RATIOS["dx_bf16"]))


@gpu
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_one_item_packer_gives_the_batched_packer_bits(kind):
    """vidc_pack_conv_weights_one against one-item launches of vidc_pack_conv_weights_batched, every kind, 3x3 and 1x1, Cin ragged against the
    packer's blocks, the parameter 4 bytes off a 16-byte boundary; nothing is written past the packed image."""
    from test_conv_backward_kernels import _pack_batched
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    for k in (3, 1):
        co, ci = (128, 76) if kind & 1 else (36, 128)              # the K side (Cout for the dgrad kinds, Cin for the forward ones) in whole units
        flat = torch.zeros(co * ci * k * k + 1)
        flat[1:] = _randn(10 * kind + k, co * ci * k * k)
        wd = flat.to(DEV)[1:]
        n = co * ci * k * k // (2 if kind & 4 else 1)              # packed size in 4-byte elements
        outs = [torch.full((n + 64,), -7777.0, device=DEV) for _ in range(2)]
        _pack_batched(L, [(wd, outs[0], co, ci, k, k, kind)])
        L.check(lib.vidc_pack_conv_weights_one(L.ptr(wd), L.ptr(outs[1]), co, ci, k, k, kind, L.current_stream()), "pack_conv_weights_one")
        torch.cuda.synchronize()
        assert _same_bits(outs[0].cpu(), outs[1].cpu()), (kind, k)
        assert bool((outs[1][n:] == -7777.0).all()) and not bool((outs[1][:n] == -7777.0).all())


@gpu
def test_ineligible_convs_take_the_fp32_gradients_bit_for_bit():
    """Cout 96 (no whole 64-channel K units): the data gradient at precision 2 is the fp32 one, bit for bit.  Cout 36 takes the fp32 path as
    well -- which has refused Cout % 32 != 0 all along (vidc_pack_conv_weight_dgrad), so there precision 2 gives precision 0's refusal, not
    bits.  Cin 6: the weight gradient is the fp32 one.  The bf16 packer refuses the shape it cannot write."""
    from vi_depth_completion_amd import ops
    dc, w, x = _randn(1, 2, 9, 11, 36).to(DEV), (_randn(2, 36, 32, 3, 3) * 0.1).to(DEV), _randn(3, 2, 9, 11, 32).to(DEV)
    assert ops.conv_backward_data_precision((36, 32, 3, 3), 2) == 0 and ops.conv_backward_data_precision((64, 36, 3, 3), 2) == 0
    assert ops.conv_backward_data_precision((96, 32, 3, 3), 2) == 0 and ops.conv_backward_data_precision((128, 32, 3, 3), 2) == 2
    assert ops.conv_backward_data_precision((64, 32, 3, 3), 1) == 1 and ops.conv_backward_data_precision((36, 32, 3, 3), 0) == 0
    dc96, w96 = _randn(6, 2, 9, 11, 96).to(DEV), (_randn(7, 96, 32, 3, 3) * 0.1).to(DEV)
    for stride, pad, shape in ((1, 1, (9, 11)), (2, 1, (5, 6))):
        g = dc96[:, :shape[0], :shape[1]].contiguous()
        assert _same_bits(ops.conv_backward_data(g, w96, 9, 11, stride, pad, 2).cpu(), ops.conv_backward_data(g, w96, 9, 11, stride, pad, 0).cpu())
    for precision in (0, 2):
        with pytest.raises(RuntimeError, match="Cout must be a multiple of 32"):
            ops.conv_backward_data(dc, w, 9, 11, 1, 1, precision)
    assert ops.conv_backward_weight_precision((36, 32, 3, 3), 2) == 2 and ops.conv_backward_weight_precision((36, 6, 3, 3), 2) == 0
    x6 = _randn(4, 2, 9, 11, 6).to(DEV)
    assert _same_bits(ops.conv_backward_weight(dc, x6, (36, 6, 3, 3), 1, 1, precision=2).cpu(), ops.conv_backward_weight(dc, x6, (36, 6, 3, 3), 1, 1).cpu())
    assert not _same_bits(ops.conv_backward_weight(dc, x, (36, 32, 3, 3), 1, 1, precision=2).cpu(), ops.conv_backward_weight(dc, x, (36, 32, 3, 3), 1, 1).cpu())
    # a contiguous view that starts 4 bytes past a 16-byte boundary: the fp32 kernel (scalar loads), with the bits it gives the aligned tensor
    flat = torch.zeros(x.numel() + 1, device=DEV)
    flat[1:] = x.reshape(-1)
    x_odd = flat[1:].view(x.shape)
    assert x_odd.is_contiguous() and x_odd.data_ptr() % 16 == 4 and ops.conv_backward_weight_precision((36, 32, 3, 3), 2, aligned=False) == 0
    assert _same_bits(ops.conv_backward_weight(dc, x_odd, (36, 32, 3, 3), 1, 1, precision=2).cpu(), ops.conv_backward_weight(dc, x, (36, 32, 3, 3), 1, 1).cpu())
    with pytest.raises(RuntimeError, match="cannot be packed for the bf16 data gradient"):
        ops.pack_conv_weight_dgrad(w, 2)
    packed = ops.pack_conv_weight_dgrad((_randn(5, 64, 32, 3, 3) * 0.1).to(DEV), 2)
    assert packed.dtype == torch.bfloat16 and packed.shape == (32, 9 * 64)
    with pytest.raises(RuntimeError, match="0 .*2"):
        ops.conv_backward_weight(dc, x, (36, 32, 3, 3), 1, 1, precision=1)


# ---- GPU: operators ----------------------------------------------------------------------------------------------------------------------
def ref_dgrad_dilated(dy, w, H, W, pad, dil):
    """ref_dgrad of a stride-1 conv whose tap (kh, kw) reads x[oy - pad + kh*dil, ox - pad + kw*dil]; dil = 1 is ref_dgrad itself."""
    if dil == 1:
        return ref_dgrad(dy, w, H, W, 1, pad)
    dy, w = dy.to(F64), w.to(F64)
    B, Co, Ho, Wo = dy.shape
    _co, Ci, KH, KW = w.shape
    dx, mag = torch.zeros(B, Ci, H + 2 * pad, W + 2 * pad, dtype=F64), torch.zeros(B, Ci, H + 2 * pad, W + 2 * pad, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            dx[:, :, kh * dil:kh * dil + Ho, kw * dil:kw * dil + Wo] += torch.einsum("bohw,oc->bchw", dy, w[:, :, kh, kw])
            mag[:, :, kh * dil:kh * dil + Ho, kw * dil:kw * dil + Wo] += torch.einsum("bohw,oc->bchw", dy.abs(), w[:, :, kh, kw].abs())
    return dx[:, :, pad:pad + H, pad:pad + W], mag[:, :, pad:pad + H, pad:pad + W]


# name -> (H, W, k, stride, pad, dilation, relu): B = 2, 64 -> 64 channels
OP_CASES = {"3x3_s1": (9, 11, 3, 1, 1, 1, False), "3x3_s2": (9, 11, 3, 2, 1, 1, False), "1x1": (9, 11, 1, 1, 0, 1, False),
            "dilated_d6": DILATED_CASES[0][:2] + (3, 1, DILATED_CASES[0][4], DILATED_CASES[0][3], False),
            "dilated_d2": DILATED_CASES[1][:2] + (3, 1, DILATED_CASES[1][4], DILATED_CASES[1][3], False),
            "3x3_s1_relu": (9, 11, 3, 1, 1, 1, True)}
assert DILATED_CASES[0] == (7, 9, 64, 6, 6) and DILATED_CASES[1] == (5, 6, 64, 2, 2)


def _op_case(name):
    H, W, k, stride, pad, dil, relu = OP_CASES[name]
    seed = 500 + sum(ord(c) for c in name)
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    x, w = _randn(seed, 2, 64, H, W), _randn(seed + 1, 64, 64, k, k) * (2.0 / (64 * k * k)) ** 0.5
    scale = torch.tensor([0.5, 1.0, 2.0, 4.0] * 16)                       # exact powers of two: dc = dy * scale is exact
    shift, dy = 0.1 * _randn(seed + 2, 64), _randn(seed + 3, 2, 64, Ho, Wo)
    return x, w, scale, shift, dy


def _op_call(name, leaves):
    _h, _w, _k, stride, pad, dil, relu = OP_CASES[name]
    if dil > 1:
        return V.conv2d_dilated_bn_act(*leaves, pad, dil, relu, 0)
    return V.conv2d_bn_act(*leaves, stride, pad, relu, 0)


def _op_grads(name, tensors, dy, grad_precision):
    """(y, [dx NHWC, dw, dscale, dshift]) of one forward + backward, the forward inside grad_precision(grad_precision) when it is not None."""
    import contextlib
    with torch.enable_grad():
        leaves = [t.clone().requires_grad_() for t in tensors]
        with (T.grad_precision(grad_precision) if grad_precision is not None else contextlib.nullcontext()):
            y = _op_call(name, leaves)
        return y.detach(), list(torch.autograd.grad((y * dy).sum(), leaves))


@gpu
@pytest.mark.parametrize("name", sorted(OP_CASES))
def test_conv_operators_inside_grad_precision_2(name):
    """x.grad and w.grad against the rounded-operand references under their bounds; scale.grad and shift.grad have the bits of grad precision 0;
    precision 2 arrives at both ops wrappers; with the context closed the operator gives the bits of its backward operator at precision 0."""
    from vi_depth_completion_amd import ops
    H, W, k, stride, pad, dil, relu = OP_CASES[name]
    x, w, scale, shift, dy = _op_case(name)
    tensors = [_nhwc(x).to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV)]
    dyd = _nhwc(dy).to(DEV)
    seen, real_w, real_x = [], ops.conv_backward_weight, ops.conv_backward_data
    ops.conv_backward_weight = lambda *a, **kw: (seen.append(("w", kw.get("precision"))), real_w(*a, **kw))[1]
    ops.conv_backward_data = lambda *a, **kw: (seen.append(("x", a[6])), real_x(*a, **kw))[1]
    try:
        y, bf = _op_grads(name, tensors, dyd, 2)
        assert sorted(seen) == [("w", 2), ("x", 2)], seen
        del seen[:]
        _y0, f32 = _op_grads(name, tensors, dyd, 0)
        assert sorted(seen) == [("w", 0), ("x", 0)], seen
    finally:
        ops.conv_backward_weight, ops.conv_backward_data = real_w, real_x
    assert T.current_grad_precision() == 0
    mask = (_nchw(y.cpu()) > 0).float() if relu else torch.ones_like(dy)                 # the operator's own forward output: the forward is not under test
    if relu:
        assert 0.2 < float(mask.mean()) < 0.8
    dc = dy * mask * scale[None, :, None, None]
    dcq, xq, wq = R.rounded(dc), R.rounded(x), R.rounded(w)
    assert not torch.equal(dcq, dc)
    want, mag = ref_dgrad_dilated(dcq, wq, H, W, pad, dil) if stride == 1 else ref_dgrad(dcq, wq, H, W, stride, pad)
    _within("op_dx_bf16", _nchw(bf[0].cpu()), want, mag, 64 * k * k + 2, name)
    M = dy.numel() // 64
    want, mag = ref_wgrad_dilated(dcq, xq, k, k, stride, pad, dil)
    _within("op_dw_bf16", bf[1].cpu(), want, mag, min(_rows_per_chunk(M, 64, 64, k * k), M) + 2, name)
    assert _same_bits(bf[2].cpu(), f32[2].cpu()) and _same_bits(bf[3].cpu(), f32[3].cpu()), "dscale / dshift changed under grad_precision(2)"
    assert not _same_bits(bf[0].cpu(), f32[0].cpu()) and not _same_bits(bf[1].cpu(), f32[1].cpu())
    # the context closed: today's backward, bit for bit -- the backward operator called directly at precision 0
    _yc, closed = _op_grads(name, tensors, dyd, None)
    if dil > 1:
        direct = V.conv2d_dilated_bn_act_backward(dyd, tensors[0], tensors[1], y, tensors[2], tensors[3], H, W, pad, dil, relu, 0, True, True, True, False)
    else:
        direct = V.conv2d_bn_act_backward(dyd, tensors[0], tensors[1], y, tensors[2], tensors[3], H, W, stride, pad, relu, 0, True, True, True, False)
    for a, b, c, what in zip(closed, direct, f32, ("dx", "dw", "dscale", "dshift")):
        assert _same_bits(a.cpu(), b.cpu().reshape(a.shape)) and _same_bits(a.cpu(), c.cpu()), what
    R_ = __import__("test_conv_backward_kernels").RATIOS
    print("\n[%s] error / bound so far: dx %.3f, dw %.3f" % (name, R_["op_dx_bf16"], R_["op_dw_bf16"]))


@gpu
def test_winograd_forward_records_grad_precision_2():
    """conv3x3_winograd at precision 1 inside grad_precision(2) hands 2 to both gradients (outside: its bf16x3 data gradient, fp32 weights)."""
    from vi_depth_completion_amd import ops
    x, w, scale, shift, dy = _op_case("3x3_s1")
    tensors = [_nhwc(x).to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV)]
    seen, real_w, real_x = [], ops.conv_backward_weight, ops.conv_backward_data
    ops.conv_backward_weight = lambda *a, **kw: (seen.append(("w", kw.get("precision"))), real_w(*a, **kw))[1]
    ops.conv_backward_data = lambda *a, **kw: (seen.append(("x", a[6])), real_x(*a, **kw))[1]
    try:
        for gp, want in ((2, [("w", 2), ("x", 2)]), (0, [("w", 0), ("x", 1)])):
            with torch.enable_grad():
                leaves = [t.clone().requires_grad_() for t in tensors]
                with T.grad_precision(gp):
                    y = V.conv3x3_winograd(*leaves, 4, False, 1)
                torch.autograd.grad((y * _nhwc(dy).to(DEV)).sum(), leaves)
            assert sorted(seen) == want, (gp, seen)
            del seen[:]
    finally:
        ops.conv_backward_weight, ops.conv_backward_data = real_w, real_x


# ---- GPU: the network --------------------------------------------------------------------------------------------------------------------
STEP_LR = 1e-3


def _flat_grad(cnn):
    return torch.cat([p.grad.double().reshape(-1) for p in cnn.parameters()])


@gpu
def test_surface_normal_network_trains_with_bf16_gradients(seeded_weights):
    """SurfaceNormalPrediction(**SMALL), B = 2: one forward_autograd + backward() at grad_precision 0 and 2 from identical state -- the losses are
    bit-identical (the forward is untouched), every parameter has a finite gradient, the flat gradients' cosine is above 0.99 and the global
    norms agree within 2e-2; then six Adam steps at each grad precision: the loss ends under 0.9 x its start and within 5 % of the fp32 steps'.
    The gradients are compared on _inputs' own target, unit-variance noise x 1.7, which no six steps fit (the fp32 loss goes 1.998 -> 1.885 at
    lr 1e-3); the steps therefore run on the learnable target of tests/test_sn_training.py::test_it_learns_in_plain_bf16, that test's lr."""
    image, gravity, aligned, noise_gt, mask = [t.to(DEV) for t in _inputs(2, 96, 128, 77, 0)]
    smooth_gt = F.normalize(torch.stack([0.4 * (image[:, 0] - 0.5), -0.6 + 0.2 * (image[:, 1] - 0.5), -0.7 + 0.0 * image[:, 2]], dim=1), dim=1) * 2.0
    grads, losses = {}, {}
    for gp in (0, 2):
        cnn = _network(seeded_weights, **SMALL)
        optimizer = torch.optim.Adam(cnn.parameters(), lr=STEP_LR)
        losses[gp] = []
        for step in range(-1, 6):                     # -1: the gradient comparison (no optimizer step, but the BatchNorms' running statistics move)
            with torch.enable_grad():
                optimizer.zero_grad()
                loss = V.normal_l1_loss(cnn.forward_autograd(image, gravity, aligned, grad_precision=gp), noise_gt if step < 0 else smooth_gt, mask, True)[0]
                loss.backward()
            losses[gp].append(loss.detach().clone())
            if step < 0:
                assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in cnn.parameters())
                grads[gp] = _flat_grad(cnn)
            else:
                optimizer.step()
        del cnn, optimizer
        torch.cuda.empty_cache()
    assert _same_bits(losses[0][0].cpu(), losses[2][0].cpu()), "the first loss differs: the forward changed"
    cos = float((grads[0] * grads[2]).sum() / (grads[0].norm() * grads[2].norm()))
    n0, n2 = float(grads[0].norm()), float(grads[2].norm())
    l0, l2 = [float(v) for v in losses[0][1:]], [float(v) for v in losses[2][1:]]
    assert _same_bits(losses[0][1].cpu(), losses[2][1].cpu())
    print("\nbf16 vs fp32 gradients: cosine %.5f, global norms %.6e vs %.6e (relative %.2e); losses fp32 %s bf16 %s" % (cos, n2, n0, abs(n2 - n0) / n0, l0, l2))
    assert cos > 0.99
    assert abs(n2 - n0) < 2e-2 * n0
    assert l2[-1] < 0.9 * l2[0]
    assert abs(l2[-1] - l0[-1]) < 0.05 * l0[-1]
    assert U == 2.0 ** -24 and _out_size(9, 3, 1, 1) == 9
