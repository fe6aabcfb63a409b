"""Training ModifiedFPN and SurfaceNormalPrediction under autograd (vi_depth_completion_amd/torch_ops.py: NET_TRAIN_OPS; networks/autograd_blocks.py and the
two modules' forward_autograd): the depth loss with its logged ratios, the use_mask multiply and the decoder's sum as differentiable torch.ops.vidc
operators -- registration, shape functions and the ratio helper on the CPU; on the GPU every new operator alone at the smallest shapes that reach its
branches, the one-channel stem, a reduced masked composition, then both networks through the reference's loop (network_run.py:231-254) with torch.optim.Adam,
alone and chained, and eval() after the step.

Bars.  Data movement, masks, counts and sign gradients are compared bit for bit with stock torch in float32 on the CPU.  The gradient bars of the row
operators and of the reduced composition are made by tests/test_torch_ops_autograd.py's own `_compare` (its header).  The depth network is held to the
assertions and constants of tests/test_training.py::test_training_iteration_vs_reference (fp32) on the same record of the reference's own iteration, the normal
network to those of tests/test_sn_training.py::test_one_iteration_vs_oracle (fp32) against the same oracle construction, the stepped modules in eval() to the
bars tests/test_hip_parity.py gives each network against the oracle (the depth test's docstring says which, and what was measured).  Where a loss computed twice in fp64 in two summation orders is rounded to fp32, the two may differ by that one rounding:
2^-24 of the value (the fp64 orders themselves differ by at most n 2^-53).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_torch_ops_autograd import _compare, _nchw, _nhwc  # noqa: E402  (the harness that file's header describes)
from test_sn_training import LR, PROBES, SMALL, STATS, _inputs  # noqa: E402  (the small network and the inputs of the normal trainer's tests)

from oracle import vidc_oracle as O  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402
from vi_depth_completion_amd import torch_ops as T  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
V = torch.ops.vidc
DELTA = 1e-3
EPS, MOMENTUM = 1e-5, 0.1
THRESHOLDS = (1.05, 1.10, 1.25, 1.25 ** 2, 1.25 ** 3)

# (B, H, W): one pixel; 182 pixels; n = 1035 and n = 3069 cross the 1024-pixel chunk of the kernel without dividing it (2 and 3 chunks)
LOSS_SHAPES = [(1, 1, 1), (2, 7, 13), (1, 23, 45), (3, 33, 31)]
# (B, h, w, C, ld, H, W): the network's level 4; a non-integer ratio with x a channel slice of a 96-wide tensor; 64 channels
MASK_CASES = [(2, 8, 10, 32, 32, 240, 320), (1, 7, 9, 32, 96, 30, 40), (2, 3, 4, 64, 64, 96, 128)]


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


# ---- restatements with stock torch ----------------------------------------------------------------------------------------------------------------
def _printable_ratios_ref(valid_gt, valid_preds):
    """GetDepthPrintableRatios (network_run.py:72-82), restated."""
    ratios = torch.max(valid_preds / valid_gt, valid_gt / valid_preds)
    out = {}
    for key, t in zip(("D_1.05", "D_1.10", "D_1.25", "D_1.56", "D_1.95"), THRESHOLDS):
        out[key] = round(100 * torch.sum(ratios < t).item() / (ratios.nelement() + 1e-7), 1)
    return out


def _depth_loss_ref(pred, gt):
    """The depth half of `_network_loss` (network_run.py:165-179) in float32 on the CPU: (loss, dpred, count, [five counts])."""
    hw = pred.shape[-2] * pred.shape[-1]
    p = pred.clone().requires_grad_()
    m = gt > 0
    with torch.enable_grad():
        loss = F.l1_loss(p[m], gt[m], reduction="sum") / hw
        loss.backward()
    r = torch.max(pred[m] / gt[m], gt[m] / pred[m])
    return loss.detach(), p.grad, int(m.sum()), [int((r < t).sum()) for t in THRESHOLDS]


def _depth_case(B, H, W):
    """About 25 % invalid pixels; valid predictions spread around the ground truth so that every threshold separates some of them."""
    seed = 100 * H + W
    gt = S.uniform01(seed, "dl.gt", (B, 1, H, W)).float() * 4 + 0.2
    gt[S.uniform01(seed, "dl.hole", (B, 1, H, W)) < 0.25] = 0.0
    pred = (gt + (gt == 0).float() * 2.0) * torch.exp(0.3 * S.normal01(seed, "dl.r", (B, 1, H, W)).float())
    return pred, gt


def _threshold_case():
    """(1, 1, 8, 12): for each threshold t and both directions, pixels at gt * float32(t) and one ulp on either side; pixels with pred == 0 and pred == gt."""
    H, W = 8, 12
    gt = (S.uniform01(5, "dl.tgt", (1, 1, H, W)).float() * 3 + 0.5).reshape(-1)
    pred = (gt * 1.3).clone()
    i = 0
    for t in THRESHOLDS:
        t32 = np.float32(t)
        for direction in (0, 1):
            g = np.float32(float(gt[i]))
            at = np.float32(g * t32) if direction == 0 else np.float32(g / t32)
            for v in (np.nextafter(at, np.float32(0)), at, np.nextafter(at, np.float32(np.inf))):
                gt[i], pred[i] = float(g), float(v)
                i += 1
    pred[i], pred[i + 1] = 0.0, 0.0                        # gt / pred = inf: below no threshold
    pred[i + 2], pred[i + 3] = gt[i + 2], gt[i + 3]        # a tie: sign(0) = 0, ratio 1
    gt[i + 4], gt[i + 5] = 0.0, -1.0                       # invalid
    assert i + 6 <= H * W
    return pred.reshape(1, 1, H, W), gt.reshape(1, 1, H, W)


def _mask_image(B, H, W, seed):
    """(B, 3, H, W) in [0, 1) with a quarter of the pixels each: r + g + b exactly float32(1e-2) (masked out: the comparison is strict), the next float
    above it, zero, and left as drawn."""
    img = S.uniform01(seed, "mask.img", (B, 3, H, W)).float()
    kind = (S.uniform01(seed, "mask.kind", (B, 1, H, W)) * 4).long().clamp_(max=3).expand(B, 3, H, W)
    edge = torch.zeros(B, 3, H, W)
    edge[:, 0] = float(np.float32(1e-2))
    above = torch.zeros(B, 3, H, W)
    above[:, 0] = float(np.nextafter(np.float32(1e-2), np.float32(1)))
    img = torch.where(kind == 0, edge, img)
    img = torch.where(kind == 1, above, img)
    return torch.where(kind == 2, torch.zeros(()), img)


def _feature_mask(image, size):
    """surface_normal.py:151-156."""
    fm = (image[:, 0:1] + image[:, 1:2] + image[:, 2:3] > 1e-2).float()
    return F.interpolate(fm, size=size, mode="nearest")


def _slice_of(xh, ld):
    """xh (NHWC) as the upper channels of a tensor `ld` wide (autograd flows through the cat and the slice)."""
    C = xh.shape[-1]
    if ld == C:
        return xh
    return torch.cat((torch.full(xh.shape[:-1] + (ld - C,), float("nan"), device=xh.device), xh), dim=3)[..., ld - C:]


def _add_case():
    return [S.normal01(31, "add.a", (2, 32, 5, 7)).float(), S.normal01(31, "add.b", (2, 32, 5, 7)).float() * 0.7 + 0.1]


def _add_ref(relu):
    def ref(a, b):
        pre = a + b
        return (F.relu(pre) if relu else pre), pre
    return ref


def _stem1_case():
    return [S.uniform01(33, "stem1.x", (2, 1, 12, 16)).float() * 4.0, S.normal01(33, "stem1.w", (64, 1, 3, 3)).float() * 0.3]


def _stem1_ref(x, w):
    pre = F.conv2d(x, w, stride=2, padding=1)
    return F.relu(pre), pre


# ---- the reduced composition: a stride-2 projection Bottleneck, the mask, a decoder branch with an upsample, the sum, the three-channel head ---------
_RED_LAYERS = [("b.conv1", (32, 64, 1, 1)), ("b.conv2", (32, 32, 3, 3)), ("b.conv3", (128, 32, 1, 1)), ("b.down", (128, 64, 1, 1)),
               ("f2.0", (64, 128, 1, 1)), ("f2.3", (64, 64, 3, 3)), ("f2.7", (32, 64, 1, 1)), ("f1.0", (32, 64, 3, 3))]
_RED_NAMES = ["x"] + [n + s for n, _shp in _RED_LAYERS for s in (".w", ".gamma", ".beta")] + ["head.w", "head.b"]


def _reduced_case():
    out = [S.normal01(41, "red.x", (2, 64, 12, 16)).float()]
    for n, shp in _RED_LAYERS:
        out += [S.normal01(41, "red.w." + n, shp).float() * (2.0 / (shp[1] * shp[2] * shp[3])) ** 0.5, 0.5 + S.uniform01(41, "red.g." + n, (shp[0],)).float(),
                0.1 * S.normal01(41, "red.b." + n, (shp[0],)).float()]
    out += [S.normal01(41, "red.hw", (3, 32, 1, 1)).float() * 0.2, 0.1 * S.normal01(41, "red.hb", (3,)).float()]
    image = _mask_image(2, 24, 32, 43)
    image[:, :, :, :9] = 0.0                                  # an empty band, as the warp leaves one
    return out, image


def _reduced_ref(image, gates=None):
    m_hi, m_lo = _feature_mask(image, (12, 16)), _feature_mask(image, (6, 8))

    def ref(x, *p):
        P = {n: p[3 * i:3 * i + 3] for i, (n, _s) in enumerate(_RED_LAYERS)}
        head_w, head_b = p[-2], p[-1]

        def cbr(t, n, stride=1, relu=True, res=None):
            w, g, b = P[n]
            y = F.batch_norm(F.conv2d(t, w, stride=stride, padding=w.shape[2] // 2), None, None, g, b, training=True, momentum=MOMENTUM, eps=EPS)
            y = y if res is None else y + res
            if relu and gates is not None:
                gates.append(y.detach())
            return F.relu(y) if relu else y

        u = cbr(cbr(x, "b.conv1"), "b.conv2", stride=2)
        t = cbr(u, "b.conv3", res=cbr(x, "b.down", stride=2, relu=False)) * m_lo.to(x.dtype)
        zb = cbr(F.interpolate(cbr(cbr(t, "f2.0"), "f2.3"), size=(12, 16), mode="bilinear", align_corners=True), "f2.7")
        za = cbr(x * m_hi.to(x.dtype), "f1.0")
        z = (za + zb) * m_hi.to(x.dtype)
        return F.interpolate(F.conv2d(z, head_w, head_b), size=(24, 32), mode="bilinear", align_corners=True), None
    return ref


def _reduced_ours(image):
    img = image.to(DEV)

    def ours(x, *p):
        P = {n: p[3 * i:3 * i + 3] for i, (n, _s) in enumerate(_RED_LAYERS)}

        def cbr(t, n, stride=1, relu=True, res=None):
            w, g, b = P[n]
            co = w.shape[0]
            c = V.conv2d_bn_act(t, w, torch.ones(co, device=DEV), torch.zeros(co, device=DEV), stride, w.shape[2] // 2, False, 0)
            return V.batch_norm_train(c, g, b, torch.zeros(co, device=DEV), torch.ones(co, device=DEV), MOMENTUM, EPS, relu, res)[0]

        xh = _nhwc(x)
        u = cbr(cbr(xh, "b.conv1"), "b.conv2", stride=2)
        t = V.feature_mask_scale(cbr(u, "b.conv3", res=cbr(xh, "b.down", stride=2, relu=False)), img)
        zb = cbr(V.upsample_bilinear_ac(cbr(cbr(t, "f2.0"), "f2.3"), 12, 16, False), "f2.7")
        za = cbr(V.feature_mask_scale(xh, img), "f1.0")
        z = V.feature_mask_scale(V.add_rows(za, zb, False), img)
        return V.head_conv1x1_upsample(z, p[-2], p[-1], 0, 24, 32, False)
    return ours


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------------------
def test_net_train_ops_are_registered():
    assert len(T.BACKWARD_OPS) == 7
    assert T.DORN_OPS == ("conv2d_dilated_bn_act", "avgpool2d") and T.DORN_BACKWARD_OPS == ("conv2d_dilated_bn_act_backward", "avgpool2d_backward")
    assert T.TRAIN_OPS == ("batch_norm_train", "dropout2d", "scale_image_channels", "normalize_nchw", "normal_l1_loss", "normal_l1_loss_with_grad")
    assert T.TRAIN_BACKWARD_OPS == ("batch_norm_train_backward", "normalize_nchw_backward", "normal_l1_loss_backward")
    for name in ("depth_l1_loss", "feature_mask_scale", "add_rows"):
        assert name in T.NET_TRAIN_OPS, name
    for name in ("depth_l1_loss_backward", "add_rows_backward"):
        assert name in T.NET_TRAIN_BACKWARD_OPS, name
    earlier = T.BACKWARD_OPS + T.DORN_OPS + T.DORN_BACKWARD_OPS + T.TRAIN_OPS + T.TRAIN_BACKWARD_OPS
    for name in T.NET_TRAIN_OPS + T.NET_TRAIN_BACKWARD_OPS:
        assert hasattr(V, name), name
        assert name in T.OPS and name not in earlier, name
    assert len(set(T.OPS)) == len(T.OPS)


def test_net_train_shape_functions():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for shape in ((2, 1, 240, 320), (2, 240, 320)):
            p = torch.empty(shape)
            loss, count, ratios = V.depth_l1_loss(p, torch.empty(shape))
            assert loss.shape == count.shape == (1,) and ratios.shape == (5,) and {t.dtype for t in (loss, count, ratios)} == {torch.float32}
            assert V.depth_l1_loss_with_grad(p, p)[3].shape == p.shape and V.depth_l1_loss_backward(p, torch.empty(1)).shape == p.shape
        x, img = torch.empty(2, 8, 10, 32), torch.empty(2, 3, 240, 320)
        assert V.feature_mask_scale(x, img).shape == x.shape
        wide = torch.empty(1, 7, 9, 96)
        y = V.feature_mask_scale(wide[..., 64:], torch.empty(1, 3, 30, 40))                 # a channel slice
        assert y.shape == (1, 7, 9, 32) and y.dtype == torch.float32
        for relu in (False, True):
            assert V.add_rows(x, x, relu).shape == x.shape and V.add_rows(wide[..., :32], wide[..., 32:64], relu).shape == (1, 7, 9, 32)
        assert V.add_rows_backward(x, x).shape == x.shape


def test_net_train_ops_carry_a_backward_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(), torch.enable_grad():
        p = torch.empty(2, 1, 24, 32, requires_grad=True)
        loss, count, ratios = V.depth_l1_loss(p, torch.empty(2, 1, 24, 32))
        assert loss.requires_grad and loss.grad_fn is not None and not count.requires_grad and not ratios.requires_grad
        assert torch.autograd.grad(loss.sum(), (p,))[0].shape == p.shape
        x = torch.empty(2, 6, 8, 32, requires_grad=True)
        img = torch.empty(2, 3, 24, 32, requires_grad=True)
        y = V.feature_mask_scale(x, img)
        assert y.grad_fn is not None
        gx, gi = torch.autograd.grad(y.sum(), (x, img), allow_unused=True)
        assert gx.shape == x.shape and gi is None                                           # the mask is detached: no gradient for the image
        b = torch.empty(2, 6, 8, 32, requires_grad=True)
        for relu in (False, True):
            ga, gb = torch.autograd.grad(V.add_rows(x, b, relu).sum(), (x, b))
            assert ga.shape == x.shape and gb.shape == b.shape
        with torch.no_grad():
            assert not V.add_rows(x, b, True).requires_grad


def test_net_train_ops_refuse_cpu_tensors():
    x, img = torch.zeros(1, 2, 2, 4), torch.ones(1, 3, 4, 4)
    calls = [lambda: V.depth_l1_loss(torch.ones(1, 1, 2, 2), torch.ones(1, 1, 2, 2)), lambda: V.depth_l1_loss_backward(torch.ones(1, 1, 2, 2), torch.ones(1)),
             lambda: V.feature_mask_scale(x, img), lambda: V.add_rows(x, x, False), lambda: V.add_rows_backward(x, x)]
    for call in calls:
        with pytest.raises((NotImplementedError, RuntimeError)):
            call()


def test_depth_printable_ratios_helper():
    """T.depth_printable_ratios(count, five counts) against GetDepthPrintableRatios restated with stock torch, on the threshold case and on seeded cases; torch
    compares the float32 ratios with the thresholds rounded to float32, so a ratio of float32(1.05) is not below 1.05."""
    assert not bool(torch.tensor([1.05]) < 1.05) and bool(torch.tensor([float(np.nextafter(np.float32(1.05), np.float32(0)))]) < 1.05)
    for pred, gt in [_threshold_case()] + [_depth_case(*s) for s in LOSS_SHAPES]:
        _loss, _dp, count, counts = _depth_loss_ref(pred, gt)
        want = _printable_ratios_ref(gt[gt > 0], pred[gt > 0])
        assert T.depth_printable_ratios(count, counts) == want
        assert T.depth_printable_ratios(torch.tensor([float(count)]), torch.tensor(counts, dtype=torch.float32)) == want
        assert list(want) == ["D_1.05", "D_1.10", "D_1.25", "D_1.56", "D_1.95"]
    assert T.depth_printable_ratios(0, [0] * 5) == {k: 0.0 for k in T.RATIO_KEYS}             # no valid pixel: 0 / 1e-7
    with pytest.raises(ValueError):
        T.depth_printable_ratios(3, [1, 2])


def test_threshold_case_separates_every_threshold():
    """The float32 restatement on the threshold case: every threshold has pixels on both sides within one ulp, so a kernel comparing in another precision or
    with another quotient would count differently."""
    pred, gt = _threshold_case()
    m = gt > 0
    r = torch.max(pred[m] / gt[m], gt[m] / pred[m])
    for t in THRESHOLDS:
        t32 = float(np.float32(t))
        near = r[(r - t32).abs() <= 2 * float(np.spacing(np.float32(t)))]
        assert bool((near < t).any()) and bool((near >= t).any()), t
    assert bool(torch.isinf(r).any()) and bool((r == 1).any()) and int((~m).sum()) == 2


def test_relu_gates_of_the_gpu_cases_stay_under_the_cap():
    """The float64 side alone: the seeded inputs of the gated GPU cases leave at most 1 % of the pre-activations within delta of zero."""
    pre = _add_ref(True)(*[t.double() for t in _add_case()])[1]
    assert (pre.abs() < DELTA).double().mean().item() <= 0.01
    pre = _stem1_ref(*[t.double() for t in _stem1_case()])[1]
    assert (pre.abs() < 5e-5).double().mean().item() <= 0.01
    tensors, image = _reduced_case()
    gates = []
    _reduced_ref(image, gates)(*[t.double() for t in tensors])
    assert len(gates) == 7
    for g in gates:
        assert (g.abs() < DELTA).double().mean().item() <= 0.01
    for size in ((12, 16), (6, 8)):
        assert 0.0 < _feature_mask(image, size).mean().item() < 1.0


def test_train_mode_forward_names_forward_autograd():
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    sn, dc = SurfaceNormalPrediction(**SMALL).train(), ModifiedFPN().train()
    with pytest.raises(RuntimeError, match="SurfaceNormalTrainer.*forward_autograd"):
        sn(torch.zeros(1, 3, 96, 128), torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="inference-only.*forward_autograd"):
        dc(torch.zeros(1, 3, 96, 128), torch.zeros(1, 3, 96, 128), torch.zeros(1, 1, 96, 128))
    with pytest.raises(RuntimeError, match="GPU only"):                                     # no CPU path
        sn.forward_autograd(torch.zeros(1, 3, 96, 128), torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        dc.forward_autograd(torch.zeros(1, 3, 96, 128), torch.zeros(1, 3, 96, 128), torch.zeros(1, 1, 96, 128))
    assert not sn._autograd_dirty and not dc._autograd_dirty


# ---- GPU: depth_l1_loss ------------------------------------------------------------------------------------------------------------------------------
def _masked_l1_loss_kernel(pred, gt):
    """vidc_masked_l1_loss (the trainer's kernel, unchanged) on GPU tensors -> (loss float64 (), dpred)."""
    from vi_depth_completion_amd import _lib as L
    n, hw = pred.numel(), pred.shape[-2] * pred.shape[-1]
    loss = torch.zeros((), dtype=torch.float64, device=DEV)
    dp, terms = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    sc = torch.empty(8 * (n // 512 + 8) + 256, dtype=torch.uint8, device=DEV)
    L.check(L.lib().vidc_masked_l1_loss(L.ptr(pred), L.ptr(gt), n, hw, L.ptr(loss), L.ptr(dp), L.ptr(terms), L.ptr(sc), L.current_stream()), "loss")
    return loss, dp.view_as(pred)


def _check_depth_loss(pred, gt):
    loss_w, dpred_w, count_w, counts_w = _depth_loss_ref(pred, gt)
    pd, gd = pred.to(DEV), gt.to(DEV)
    with torch.enable_grad():
        p = pd.clone().requires_grad_()
        loss, count, ratios = V.depth_l1_loss(p, gd)
        assert loss.shape == count.shape == (1,) and ratios.shape == (5,) and loss.requires_grad and not count.requires_grad and not ratios.requires_grad
        (loss * 0.37).sum().backward()
    loss = loss.detach()
    print("depth_l1_loss %s: loss %.9g vs %.9g, count %d, ratios %s" % (tuple(pred.shape), float(loss), float(loss_w), int(count), ratios.tolist()))
    assert count.item() == count_w and ratios.tolist() == [float(c) for c in counts_w]
    assert abs(float(loss) - float(loss_w)) <= 1e-6 * float(loss_w)
    _l, _c, _r, dpred = V.depth_l1_loss_with_grad(pd, gd)
    assert torch.equal(dpred.cpu(), dpred_w) and (count_w == 0 or dpred.abs().max() > 0)
    assert torch.equal(p.grad, dpred * 0.37)                                                 # a non-unit grad_loss scales dpred: one float32 product
    loss64, dpred_k = _masked_l1_loss_kernel(pd, gd)
    assert torch.equal(dpred.view(torch.int32), dpred_k.view(torch.int32))
    assert abs(float(loss) - float(loss64)) <= 2.0 ** -24 * (1 + 1e-3) * float(loss64)       # two fp64 orders, one rounding to float32 (the header)
    again = V.depth_l1_loss_with_grad(pd, gd)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((_l, _c, _r, dpred), again))
    return loss, count, ratios


@gpu
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_ids(LOSS_SHAPES))
def test_depth_l1_loss_operator(shape):
    _loss, count, _ratios = _check_depth_loss(*_depth_case(*shape))
    assert count.item() > 0


@gpu
def test_depth_l1_loss_at_the_thresholds_and_without_valid_pixels():
    pred, gt = _threshold_case()
    _check_depth_loss(pred, gt)
    loss, count, ratios = _check_depth_loss(pred, torch.zeros_like(gt))
    assert loss.item() == 0.0 and count.item() == 0.0 and not ratios.any()
    loss, count, ratios = V.depth_l1_loss(pred.to(DEV)[:, 0], gt.to(DEV)[:, 0])              # (B, H, W) inputs
    assert count.item() == float((gt > 0).sum())


# ---- GPU: feature_mask_scale ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", MASK_CASES, ids=_ids(MASK_CASES))
def test_feature_mask_scale_operator(case):
    from vi_depth_completion_amd import ops
    B, h, w, C, ld, H, W = case
    x = S.normal01(51, "mask.x", (B, C, h, w)).float()
    dy = S.normal01(51, "mask.dy", (B, C, h, w)).float()
    image = _mask_image(B, H, W, 52)
    mask = _feature_mask(image, (h, w))
    assert 0.0 < mask.mean().item() < 1.0
    with torch.enable_grad():
        xr = x.clone().requires_grad_()
        want = xr * mask
        (want * dy).sum().backward()
        xd, img = x.to(DEV).requires_grad_(), image.to(DEV).requires_grad_()
        xs = _slice_of(_nhwc(xd), ld)
        assert ops._rows(xs)[3] == ld and ops._rows(xs)[0].data_ptr() == xs.data_ptr()      # no dense copy is made of the slice
        y = V.feature_mask_scale(xs, img)
        (_nchw(y) * dy.to(DEV)).sum().backward()
    assert y.shape == (B, h, w, C) and y.is_contiguous()
    assert torch.equal(_nchw(y).detach().cpu(), want.detach())
    assert torch.equal(xd.grad.cpu(), xr.grad) and img.grad is None


# ---- GPU: add_rows and the one-channel stem ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("relu", [False, True])
def test_add_rows_operator(relu):
    """M = 70 rows of 32 channels, both summands channel slices of 128-wide tensors."""
    from vi_depth_completion_amd import ops
    a, b = _add_case()
    seen = {}

    def ours(a_, b_):
        sa, sb = _slice_of(_nhwc(a_), 128), _slice_of(_nhwc(b_), 128)
        assert ops._rows(sa)[3] == 128 and ops._rows(sa)[0].data_ptr() == sa.data_ptr()
        seen["y"] = V.add_rows(sa, sb, relu)
        return _nchw(seen["y"])

    _compare("add_rows[relu=%d]" % relu, _add_ref(relu), ours, [a, b], ["a", "b"], delta=DELTA if relu else None)
    want = a + b
    assert torch.equal(_nchw(seen["y"]).detach().cpu(), F.relu(want) if relu else want)


@gpu
def test_stem_conv_with_one_input_channel_gradient():
    """The depth pyramid's stem: Conv2d(1, 64, 3, 2, 1) + ReLU on (2, 1, 12, 16); delta as tests/test_torch_ops_autograd.py gives the stem."""
    _compare("stem_conv3x3s2[cin=1]", _stem1_ref, lambda t, wt: _nchw(V.stem_conv3x3s2(t, wt, True)), _stem1_case(), ["x", "w"], delta=5e-5)


# ---- GPU: the reduced composition ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_reduced_masked_decoder_matches_float64_restatement():
    tensors, image = _reduced_case()
    _compare("reduced-net", _reduced_ref(image), _reduced_ours(image), tensors, _RED_NAMES, how="l1")


# ---- GPU: the networks --------------------------------------------------------------------------------------------------------------------------------
def _load(cnn, weights):
    st = cnn.state_dict()
    st.update({k: v.to(DEV) for k, v in weights.items()})
    cnn.load_state_dict(st)
    return cnn


def _dc_network(seeded_weights):
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    return _load(ModifiedFPN().to(DEV), seeded_weights["dc"])


def _sn_network(seeded_weights, **kw):
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    return _load(SurfaceNormalPrediction(**kw).to(DEV), seeded_weights["sn"])


def _train_fixture(golden_dir):
    """The inputs of tests/golden/train_step.npz, as tests/test_training.py builds them."""
    f = np.load(os.path.join(golden_dir, "train_step.npz"))
    batch = S.synthetic_batch(2, 240, 320, 1234, frame0=int(f["frame0"]))
    gt = S.synthetic_ground_truth_depth(batch["image"], 1234)
    din = torch.zeros(2, 240, 320)
    rc = torch.from_numpy(f["depth_in_rc"]).long()
    din[rc[:, 0], rc[:, 1], rc[:, 2]] = torch.from_numpy(f["depth_in_val"])
    return f, batch["image"], torch.from_numpy(f["normal"]), din[:, None], gt


def _grad_norm(cnn):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in cnn.parameters())))


@gpu
def test_depth_network_trains_through_the_reference_loop(golden_dir, seeded_weights, monkeypatch):
    """The reference's own `_run_training_iteration` at B = 2, 240 x 320 (tests/golden/train_step.npz): ModifiedFPN.forward_autograd + depth_l1_loss + backward() +
    torch.optim.Adam, with the fp32 assertions and constants of tests/test_training.py::test_training_iteration_vs_reference -- loss, prediction probe, global
    gradient norm, the 29 probed gradients, the stepped parameters, the running statistics; the ratios against the float32 restatement on the prediction.

    Then eval(): not the output before the step, and the oracle on the updated state_dict within the bars tests/test_hip_parity.py gives this network against the
    oracle -- RMSE 1e-3 in the default (mixed) arithmetic (test_full_path_vs_oracle_batch2; smoke()'s bar), as tests/test_dorn_autograd_training.py takes
    test_hip_dorn_vs_oracle's for DORN -- and, re-folded once more in the reference's arithmetic (VIDC_PRECISION=fp32), within that file's fp32 bars for this network
    (RMSE 2e-5, max 2e-4: test_depth_completion_net_teacher_forced).  Measured on an MI355X: fp32 RMSE 1.2e-6, max 5.0e-6; mixed RMSE 1.13e-4, max 1.6e-4, nearly all
    of it a uniform offset of -1.1e-4 m on a 3.1 m map -- above the 1e-4 that file's mixed mode keeps against the reference's own output on the seeded weights
    (1.5e-5 here before the step).  A fresh module loaded with the updated state_dict gives the same bits, so nothing stale is left behind: the offset is the mixed
    inference program's own arithmetic on the stepped weights (the first Adam step moves every weight by lr in the direction of its gradient, and this network turns
    that into a 0.64 m change of the mean depth)."""
    from _probe import check_probe
    f, image, normal, depth_in, gt = _train_fixture(golden_dir)
    cnn = _dc_network(seeded_weights)
    ins1 = [t[:1].to(DEV) for t in (image, normal, depth_in)]
    with torch.no_grad():
        before = cnn.eval()(*ins1).cpu()
    cnn.train()
    lr = float(f["lr"])
    optimizer = torch.optim.Adam(cnn.parameters(), lr=lr)
    with torch.enable_grad():
        optimizer.zero_grad()
        pred = cnn.forward_autograd(image.to(DEV), normal.to(DEV), depth_in.to(DEV))
        loss, count, ratios = V.depth_l1_loss(pred, gt.to(DEV))
        loss.backward()
    assert pred.shape == (2, 1, 240, 320) and cnn._autograd_dirty
    loss = float(loss.detach())
    pred_c = pred.detach().cpu()
    print("depth net: loss %.8f vs %.8f, ratios %s" % (loss, float(f["loss"]), T.depth_printable_ratios(count, ratios)))
    assert abs(loss - float(f["loss"])) < 2e-5 * float(f["loss"]), (loss, float(f["loss"]))
    assert round(loss, 4) == float(f["loss_logged"])
    assert np.abs(pred_c[:, 0, ::16, ::16].numpy() - f["pred_probe"]).max() < 1e-3
    _l, _d, count_w, counts_w = _depth_loss_ref(pred_c, gt)
    assert count.item() == count_w and ratios.tolist() == [float(c) for c in counts_w]
    assert T.depth_printable_ratios(count, ratios) == _printable_ratios_ref(gt[gt > 0], pred_c[gt > 0])
    gn = _grad_norm(cnn)
    assert abs(gn - float(f["grad_global_norm"])) < 1e-3 * gn, (gn, float(f["grad_global_norm"]))
    param = dict(cnn.named_parameters())
    names = sorted({k.split("|")[1] for k in f.files if k.startswith("grad|")})
    assert len(names) == 29
    for k in names:
        if k in ("feature1_upsamping.0.bias", "feature4_upsamping.14.bias"):          # bias in front of a BatchNorm: exact gradient 0
            assert float(param[k].grad.abs().max()) < 1e-5, k
            continue
        tight = k.startswith("feature_concat") or k in ("feature1_upsamping.4.weight", "feature1_upsamping.0.weight")
        check_probe(f, "grad", k, param[k].grad.cpu(), 5e-4 if tight else 2e-2, 1e-7)
    optimizer.step()
    n_certain = 0
    for k in names:                                                                    # (that test's reading of the first Adam step)
        key, t = "|%s|" % k, param[k].detach().cpu().reshape(-1)
        if "new" + key + "full" in f.files:
            new, gref, got = f["new" + key + "full"], f["grad" + key + "full"], t.numpy()
        else:
            new, gref, got = f["new" + key + "val"], f["grad" + key + "val"], t[torch.from_numpy(f["new" + key + "idx"])].numpy()
        assert np.abs(got - new).max() < 2.1 * lr, (k, np.abs(got - new).max())
        if np.abs(gref).max() < 1e-7:
            continue
        certain = np.abs(gref) > 0.05 * np.abs(gref).max()
        n_certain += int(certain.sum())
        assert np.abs(got - new)[certain].max() < 1e-6, (k, np.abs(got - new)[certain].max())
        old = f["old" + key + ("full" if "old" + key + "full" in f.files else "val")]
        assert np.abs(np.abs(got - old)[certain] - lr).max() < 2e-6, k
    assert n_certain > 1000
    sd = cnn.state_dict()
    for k in [k[4:] for k in f.files if k.startswith("buf|")]:
        assert np.abs(sd[k].cpu().numpy() - f["buf|" + k]).max() < 1e-4 * max(1.0, np.abs(f["buf|" + k]).max()), k
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    with torch.no_grad():
        after = cnn.eval()(*ins1).cpu()
    assert not cnn._autograd_dirty
    want = O.depth_completion_forward({k: v.detach().cpu() for k, v in sd.items()}, image[:1], normal[:1], depth_in[:1])
    d = (after - want).abs()
    print("depth net in eval() after the step: RMSE %.3e, max %.3e vs the oracle" % (float(d.pow(2).mean().sqrt()), float(d.max())))
    assert float(d.pow(2).mean().sqrt()) < 1e-3
    assert not torch.equal(after, before)
    monkeypatch.setenv("VIDC_PRECISION", "fp32")
    cnn._invalidate()
    with torch.no_grad():
        d = (cnn(*ins1).cpu() - want).abs()
    print("... and in fp32 arithmetic: RMSE %.3e, max %.3e" % (float(d.pow(2).mean().sqrt()), float(d.max())))
    assert float(d.pow(2).mean().sqrt()) < 2e-5 and float(d.max()) < 2e-4


_SN_ORACLE = {}


def _sn_oracle_iteration(seeded_weights, use_mask):
    """One iteration of the SMALL network at B = 2 on the CPU, as tests/test_sn_training.py's `oracle_iteration` builds it: oracle.vidc_oracle's
    surface_normal_forward(use_mask=...) under train-mode BatchNorm with the parameters as leaves, the loss of network_run.py:182-189 restated, backward,
    oracle.train_oracle.adam_step.  Computed once per use_mask and shared."""
    if use_mask not in _SN_ORACLE:
        from oracle import train_oracle as TO
        intr = O.Intrinsics(float(SMALL["fc_img"][0]), float(SMALL["fc_img"][1]), float(SMALL["cc_img"][0]), float(SMALL["cc_img"][1]))
        assert (intr.H, intr.W) == tuple(SMALL["output_size"])
        ins = _inputs(2, 96, 128, 77, 0)
        image, gravity, aligned, normal_gt, mask = ins
        work = {k: (v.detach().clone().requires_grad_(True) if TO.is_parameter(k) else v.detach().clone()) for k, v in seeded_weights["sn"].items()}
        with torch.enable_grad(), TO.bn_training():
            pred = O.surface_normal_forward(work, image, gravity, aligned, intr, use_mask=use_mask)
            m = (mask > 0).float()[:, None]
            gh = F.normalize(normal_gt)
            n = F.normalize(pred, dim=1)
            loss = F.l1_loss(n * m, gh * m, reduction="sum") / m.sum()
            angle = (torch.acos(torch.clamp((n * gh).sum(1, keepdim=True), -1, 1)) / np.pi * 180 * m).sum()
            loss.backward()
        params = {k: v.detach() for k, v in work.items() if v.requires_grad}
        grads = {k: work[k].grad for k in params}
        new = TO.adam_step(params, grads, {}, LR)
        gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
        _SN_ORACLE[use_mask] = {"ins": ins, "intr": intr, "loss": float(loss.detach()), "angle": float(angle.detach()), "grad_norm": gn,
                                "new": {k: new[k] for k in PROBES}, "stats": {k: work[k] for k in STATS}}
    return _SN_ORACLE[use_mask]


@gpu
@pytest.mark.parametrize("use_mask", [False, True])
def test_normal_network_trains_through_the_reference_loop(seeded_weights, use_mask):
    """SurfaceNormalPrediction(use_mask=...) at SMALL, B = 2: forward_autograd + normal_l1_loss + backward() + torch.optim.Adam against the CPU oracle with the fp32 bars
    of tests/test_sn_training.py::test_one_iteration_vs_oracle (loss 1e-5, gradient norm 1e-3, angle 1e-3, the probed parameters within 2.1 lr, the running
    statistics within 1e-4 max(1, |ref|), num_batches_tracked == 1); with use_mask the warped image does contain masked pixels; then eval(): the oracle on the
    updated state_dict within tests/test_hip_parity.py's oracle bars for this network (max 2e-3, mean 5e-5), and not the output before the step."""
    ref = _sn_oracle_iteration(seeded_weights, use_mask)
    cnn = _sn_network(seeded_weights, use_mask=use_mask, **SMALL)
    image, gravity, aligned, normal_gt, mask = [t.to(DEV) for t in ref["ins"]]
    with torch.no_grad():
        before = cnn.eval()(image, gravity, aligned).cpu()
    cnn.train()
    if use_mask:
        wp = cnn.warp_2dof_alignment
        xw = V.warp2dof_fwd(image, gravity, aligned, wp.fx, wp.fy, wp.cx, wp.cy, wp.align_corners)[1]
        fm = _feature_mask(xw.cpu(), (24, 32))
        print("use_mask: %.1f %% of the level-1 positions are kept" % (100 * fm.mean().item()))
        assert 0.0 < fm.mean().item() < 1.0
    optimizer = torch.optim.Adam(cnn.parameters(), lr=LR)
    with torch.enable_grad():
        optimizer.zero_grad()
        out = cnn.forward_autograd(image, gravity, aligned)
        loss, count, angle = V.normal_l1_loss(out, normal_gt, mask, True)
        loss.backward()
    assert out.shape == (2, 3, 96, 128) and out.grad_fn is not None
    gn, loss = _grad_norm(cnn), loss.detach()
    print("normal net (use_mask=%d): loss %.8f vs %.8f, angle %.3f vs %.3f, grad norm %.6e vs %.6e"
          % (use_mask, float(loss), ref["loss"], float(angle), ref["angle"], gn, ref["grad_norm"]))
    assert abs(float(loss) - ref["loss"]) < 1e-5 * ref["loss"]
    assert abs(gn - ref["grad_norm"]) < 1e-3 * gn
    assert abs(float(angle) - ref["angle"]) < 1e-3 * ref["angle"]
    assert float(count) == float((ref["ins"][4] > 0).sum())
    optimizer.step()
    sd = cnn.state_dict()
    for k in PROBES:
        err = float((sd[k].cpu() - ref["new"][k]).abs().max())
        print("%s after the step: max|diff| %.3e (lr %.0e)" % (k, err, LR))
        assert err < 2.1 * LR, k
    for k in STATS:
        want = ref["stats"][k]
        assert float((sd[k].cpu() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), k
    assert int(sd["resnet_pyramids.bn1.num_batches_tracked"]) == 1
    with torch.no_grad():
        after = cnn.eval()(image, gravity, aligned).cpu()
    want = O.surface_normal_forward({k: v.detach().cpu() for k, v in sd.items()}, *ref["ins"][:3], ref["intr"], use_mask=use_mask)
    d = (after - want).abs()
    print("normal net in eval() after the step: max %.3e, mean %.3e vs the oracle" % (float(d.max()), float(d.mean())))
    assert float(d.max()) < 2e-3 and float(d.mean()) < 5e-5
    assert not torch.equal(after, before)


@gpu
def test_joint_step_reaches_the_normal_network(seeded_weights):
    """Both networks in train() at SMALL, B = 2 (RunDepthCompletion's `_call_cnn` without the plane block): the normals of SurfaceNormalPrediction.forward_autograd
    feed ModifiedFPN.forward_autograd and the depth loss is backpropagated.  Every parameter of both networks gets a finite gradient, the normal network's are
    not all zero, a second run gives the same loss bits, and with resnet_rgb frozen its parameters get no .grad while every other gradient keeps its bits."""
    sn, dc = _sn_network(seeded_weights, **SMALL).train(), _dc_network(seeded_weights).train()
    image, gravity, aligned, _gt, _mask = [t.to(DEV) for t in _inputs(2, 96, 128, 77, 0)]
    batch = S.synthetic_batch(2, 96, 128, 77, frame0=0)
    depth_in, gt = batch["sparse_depth"].to(DEV), S.synthetic_ground_truth_depth(batch["image"], 77).to(DEV)

    def step():
        for p in list(sn.parameters()) + list(dc.parameters()):
            p.grad = None
        with torch.enable_grad():
            normals = sn.forward_autograd(image, gravity, aligned)
            loss = V.depth_l1_loss(dc.forward_autograd(image, normals, depth_in), gt)[0]
            loss.backward()
        return loss.detach().clone(), {("sn." if m is sn else "dc.") + n: p.grad for m in (sn, dc) for n, p in m.named_parameters()}

    loss1, g1 = step()
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in g1.values()), [n for n, g in g1.items() if g is None or not bool(torch.isfinite(g).all())][:5]
    assert sum(float(g.abs().sum()) for n, g in g1.items() if n.startswith("sn.")) > 0
    assert any(float(g.abs().max()) > 0 for n, g in g1.items() if n.startswith("sn.resnet_pyramids.conv1."))
    loss2, g2 = step()
    assert torch.equal(loss1.view(torch.int32), loss2.view(torch.int32)) and bool(torch.isfinite(loss1).all())
    assert all(torch.equal(g1[n], g2[n]) for n in g1)
    dc.resnet_rgb.requires_grad_(False)
    loss3, g3 = step()
    assert torch.equal(loss1.view(torch.int32), loss3.view(torch.int32))
    frozen = [n for n in g3 if n.startswith("dc.resnet_rgb.")]
    assert len(frozen) > 300 and all(g3[n] is None for n in frozen)
    assert all(torch.equal(g1[n].view(torch.int32), g3[n].view(torch.int32)) for n in g3 if n not in frozen)
    assert int(sn.resnet_pyramids.bn1.num_batches_tracked) == 3 and int(dc.resnet_depth.bn1.num_batches_tracked) == 3


@gpu
def test_precision_1_steps_stay_finite_and_keep_the_loss(golden_dir, seeded_weights):
    """One step of each network with the convs in bf16x3 (precision=1): every gradient finite, and the loss within the bar the two iteration tests give that mode:
    2e-5 of the reference's recorded loss (depth) and of the oracle's (normal)."""
    f, image, normal, depth_in, gt = _train_fixture(golden_dir)
    dc = _dc_network(seeded_weights).train()
    with torch.enable_grad():
        loss = V.depth_l1_loss(dc.forward_autograd(image.to(DEV), normal.to(DEV), depth_in.to(DEV), precision=1), gt.to(DEV))[0]
        loss.backward()
    loss = loss.detach()
    print("depth net, bf16x3: loss %.8f vs %.8f" % (float(loss), float(f["loss"])))
    assert abs(float(loss) - float(f["loss"])) < 2e-5 * float(f["loss"])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in dc.parameters())
    del dc, loss
    ref = _sn_oracle_iteration(seeded_weights, False)
    sn = _sn_network(seeded_weights, **SMALL).train()
    image, gravity, aligned, normal_gt, mask = [t.to(DEV) for t in ref["ins"]]
    with torch.enable_grad():
        loss = V.normal_l1_loss(sn.forward_autograd(image, gravity, aligned, precision=1), normal_gt, mask, True)[0]
        loss.backward()
    loss = loss.detach()
    print("normal net, bf16x3: loss %.8f vs %.8f" % (float(loss), ref["loss"]))
    assert abs(float(loss) - ref["loss"]) < 2e-5 * ref["loss"]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in sn.parameters())
    with pytest.raises(RuntimeError, match="precision"):
        sn.forward_autograd(image, gravity, aligned, precision=2)
