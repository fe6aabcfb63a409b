"""Fine-tuning under autograd with frozen BatchNorm: torch.ops.vidc.batch_norm_eval (vi_depth_completion_amd/torch_ops.py: FROZEN_BN_OPS) and the
per-module dispatch of networks/autograd_blocks.py's Walk.bn -- `net.train()`, then `m.eval()` on any subset of the BatchNorm2d modules.

CPU: registration, shape functions, a backward under fake tensors, the CPU refusal, and the float64 side of the operator case (its ambiguous ReLU
gates stay under the 1 % cap).  GPU: the operator through autograd against float64 torch under the counted bounds of tests/test_bn_eval_kernels.py (its
header derives them); then the networks: SurfaceNormalPrediction at tests/test_sn_training.py's SMALL size with every BatchNorm frozen and with the pyramids'
only, against oracle.vidc_oracle differentiated with eval-mode BatchNorm (where frozen) at the fp32 bars of test_one_iteration_vs_oracle; nothing frozen
against the walk as it was before the dispatch, bit for bit; SurfaceNormalDORN with every BatchNorm frozen against the float64 restatement of
tests/test_dorn_autograd_training.py with F.batch_norm(training=False), at that file's bars.  Measured figures: profiles/EXPERIMENTS.md.
"""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bn_eval_kernels import K_DBETA, K_DGAMMA, K_DX, K_Y, ref_backward, ref_forward  # noqa: E402  (the float64 references and the counted factors)
from test_train_kernels import F64, U  # noqa: E402
from test_torch_ops_autograd import _compare  # noqa: E402
from test_sn_training import LR, SMALL, _inputs  # noqa: E402
from test_net_autograd_training import _grad_norm, _sn_network  # noqa: E402
from test_dorn_autograd_training import _dorn_case, _masked_l1  # noqa: E402

from oracle import vidc_oracle as O  # noqa: E402
from vi_depth_completion_amd import torch_ops as T  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
V = torch.ops.vidc
EPS = 1e-5
OP_SHAPE = (3, 7, 9, 68)                       # M = 189 rows: no multiple of 16 or 64; 68 channels: a partial second channel block


def _freeze(module, prefix=""):
    """The usual idiom: every BatchNorm2d under `module` whose qualified name starts with `prefix` into eval() mode.  Returns their names."""
    names = []
    for n, m in module.named_modules():
        if isinstance(m, nn.BatchNorm2d) and n.startswith(prefix):
            m.eval()
            names.append(n)
    return names


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype).cpu()


def _stat_bits(module):
    return {n: _bits(b).clone() for n, b in module.named_buffers() if n.endswith(("running_mean", "running_var", "num_batches_tracked"))}


# ---- the operator case ---------------------------------------------------------------------------------------------------------------------------
def _op_case():
    g = torch.Generator().manual_seed(680)
    B, H, W, C = OP_SHAPE
    M = B * H * W
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    res, dy = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    f = ref_forward(x, gamma, beta, rm, rv, float(torch.tensor(EPS)), 1, res)
    ambiguous = f["pre"].abs() <= K_Y * U * f["y_mag"]          # the kernel's fp32 pre-activation may fall on either side of 0
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, fwd=f, ambiguous=ambiguous)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------------------
def test_frozen_bn_ops_are_registered():
    assert T.FROZEN_BN_OPS == ("batch_norm_eval",) and T.FROZEN_BN_BACKWARD_OPS == ("batch_norm_eval_backward",)
    for name in T.FROZEN_BN_OPS + T.FROZEN_BN_BACKWARD_OPS:
        assert hasattr(V, name) and name in T.OPS, name
    assert len(set(T.OPS)) == len(T.OPS)
    schema = str(V.batch_norm_eval.default._schema)
    assert "!" not in schema and "Tensor? residual=None" in schema, schema                     # nothing is mutated: the running statistics are read only


def test_frozen_bn_carries_a_backward_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(), torch.enable_grad():
        x, r = torch.empty(OP_SHAPE, requires_grad=True), torch.empty(OP_SHAPE, requires_grad=True)
        g, b = torch.empty(68, requires_grad=True), torch.empty(68, requires_grad=True)
        rm, rv = torch.empty(68), torch.empty(68)
        for relu in (False, True):
            y = V.batch_norm_eval(x, g, b, rm, rv, EPS, relu, r)
            assert y.shape == x.shape and y.dtype == torch.float32 and y.requires_grad and y.grad_fn is not None
            assert [t.shape for t in torch.autograd.grad(y.sum(), (x, g, b, r))] == [x.shape, g.shape, b.shape, r.shape]
            y = V.batch_norm_eval(x, g, b, rm, rv, EPS, relu)
            assert [t.shape for t in torch.autograd.grad(y.sum(), (x, g, b))] == [x.shape, g.shape, b.shape]
        wide = torch.empty(3, 7, 9, 128)
        assert V.batch_norm_eval(wide[..., 60:], g, b, rm, rv, EPS, True).shape == OP_SHAPE                # a channel slice
        y = V.batch_norm_eval(x, g.detach(), b.detach(), rm, rv, EPS, True)                                # frozen affine parameters
        assert torch.autograd.grad(y.sum(), (x,))[0].shape == x.shape
        dx, dg, db, dr = V.batch_norm_eval_backward(y, x, y, g, rm, rv, EPS, True, True, True)
        assert dx.shape == x.shape and dg.shape == (68,) and db.shape == (68,) and dr.shape == x.shape
        dx, dg, db, dr = V.batch_norm_eval_backward(y, None, None, g, rm, rv, EPS, True, False, False)
        assert dx.numel() == dg.numel() == db.numel() == dr.numel() == 0
        with torch.no_grad():
            assert not V.batch_norm_eval(x, g, b, rm, rv, EPS, True).requires_grad


def test_frozen_bn_refuses_cpu_tensors():
    x, c = torch.zeros(1, 2, 2, 4), torch.ones(4)
    for call in (lambda: V.batch_norm_eval(x, c, c, c, c, EPS, True), lambda: V.batch_norm_eval(x, c, c, c, c, EPS, False, x),
                 lambda: V.batch_norm_eval_backward(x, x, None, c, c, c, EPS, False, True, True)):
        with pytest.raises((NotImplementedError, RuntimeError)):
            call()


def test_operator_case_keeps_its_gates_under_the_cap():
    """From the reference alone: at most 1 % of the elements of the GPU operator case have a float64 pre-activation within the forward bound of 0 (they
    are left out of the gradient comparison), and both sides of the ReLU are populated."""
    c = _op_case()
    frac = float(c["ambiguous"].double().mean())
    print("ambiguous gates: %.4f %%" % (100 * frac))
    assert frac <= 0.01
    assert 0.2 < float((c["fwd"]["pre"] > 0).double().mean()) < 0.8


def test_walk_dispatches_per_module_and_refuses_untracked_statistics():
    """Walk.bn without a GPU: a module in eval() mode goes to batch_norm_eval with (weight, bias, running statistics, eps, relu, residual) and adds no
    counter; one in train() mode goes to batch_norm_train and adds its num_batches_tracked; track_running_stats=False is refused in either mode."""
    from vi_depth_completion_amd.networks import autograd_blocks as AB
    calls = []

    class _Ops:
        def batch_norm_eval(self, *a):
            calls.append(("eval",) + a)
            return "y_eval"

        def batch_norm_train(self, *a):
            calls.append(("train",) + a)
            return ("y_train", None, None)

    walk = AB.Walk("test", "cpu", 0)
    walk.V = _Ops()
    m = nn.BatchNorm2d(8)
    t, r = torch.zeros(1, 2, 2, 8), torch.ones(1, 2, 2, 8)
    assert walk.bn(t, m, True, r) == "y_train" and walk._counters == [m.num_batches_tracked]
    m.eval()
    assert walk.bn(t, m, True, r) == "y_eval" and len(walk._counters) == 1
    kind, a_t, a_w, a_b, a_rm, a_rv, a_eps, a_relu, a_res = calls[1]
    assert kind == "eval" and a_t is t and a_w is m.weight and a_b is m.bias and a_rm is m.running_mean and a_rv is m.running_var
    assert a_eps == m.eps and a_relu is True and a_res is r
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="running statistics"):
            walk.bn(t, nn.BatchNorm2d(8, track_running_stats=False).train(mode), False)
    AB.Walk("test", "cpu", 0).finish()                     # no counters (every BatchNorm frozen): nothing to bump, no error


# ---- GPU: the operator through autograd ----------------------------------------------------------------------------------------------------------------
def _within(name, got, want, mag, factor):
    err = (got.detach().cpu().to(F64) - want).abs()
    bound = factor * U * mag
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    print("batch_norm_eval %-10s error / bound %.3f" % (name, float(ratio.max())))
    assert float(ratio.max()) <= 1.0, (name, float(ratio.max()))


@gpu
def test_operator_through_autograd_vs_float64():
    """(3, 7, 9, 68) with a residual and a ReLU: y, dx, dgamma, dbeta against float64 under the counted bounds of tests/test_bn_eval_kernels.py, dresidual
    the masked gradient itself (exact); dy is zeroed where the gate is ambiguous.  With gamma and beta frozen: .grad is None for both, the same dx bits, x not
    handed to the backward, no scratch allocated and so no reduction launched."""
    from vi_depth_completion_amd import ops
    c = _op_case()
    shape = OP_SHAPE
    dy = c["dy"].masked_fill(c["ambiguous"], 0.0)
    b = ref_backward(dy, c["x"], c["fwd"]["y"], c["gamma"], c["rm"], c["rv"], float(torch.tensor(EPS)))
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    stat_bits = (_bits(rm).clone(), _bits(rv).clone())

    def leaves(affine):
        x, res = c["x"].reshape(shape).to(DEV).requires_grad_(True), c["res"].reshape(shape).to(DEV).requires_grad_(True)
        return x, c["gamma"].to(DEV).requires_grad_(affine), c["beta"].to(DEV).requires_grad_(affine), res

    seen = []
    real, real_scratch = ops.batch_norm_eval_backward, ops._scratch
    ops.batch_norm_eval_backward = lambda *a: (seen.append(("call", a[1] is None, a[8], a[9])), real(*a))[1]
    ops._scratch = lambda *a: (seen.append(("scratch",)), real_scratch(*a))[1]
    try:
        with torch.enable_grad():
            x, gamma, beta, res = leaves(True)
            y = V.batch_norm_eval(x, gamma, beta, rm, rv, EPS, True, res)
            (y * dy.reshape(shape).to(DEV)).sum().backward()
            full_calls, seen[:] = list(seen), []
            x2, gamma2, beta2, res2 = leaves(False)
            y2 = V.batch_norm_eval(x2, gamma2, beta2, rm, rv, EPS, True, res2)
            (y2 * dy.reshape(shape).to(DEV)).sum().backward()
    finally:
        ops.batch_norm_eval_backward, ops._scratch = real, real_scratch
    M = c["x"].shape[0]
    _within("y", y.reshape(M, -1), c["fwd"]["y"], c["fwd"]["y_mag"], K_Y)
    _within("dx", x.grad.reshape(M, -1), b["dx"], b["dx_mag"], K_DX)
    _within("dgamma", gamma.grad, b["dgamma"], b["dgamma_mag"], K_DGAMMA)
    _within("dbeta", beta.grad, b["dbeta"], b["dbeta_mag"], K_DBETA)
    want_res = (dy.to(F64) * (c["fwd"]["pre"] > 0).to(F64)).float()
    assert torch.equal(res.grad.reshape(M, -1).cpu(), want_res), "dresidual is the masked gradient itself"
    assert full_calls == [("call", False, True, True), ("scratch",)], full_calls
    assert seen == [("call", True, True, False)], seen                      # x not saved, no scratch: the reduction cannot have been launched
    assert gamma2.grad is None and beta2.grad is None
    assert torch.equal(_bits(x2.grad), _bits(x.grad)) and torch.equal(_bits(res2.grad), _bits(res.grad)) and torch.equal(_bits(y2), _bits(y))
    assert torch.equal(_bits(rm), stat_bits[0]) and torch.equal(_bits(rv), stat_bits[1])
    with torch.enable_grad():                                                # x needs no gradient: no dx is written
        seen_dx = []
        ops.batch_norm_eval_backward = lambda *a: (seen_dx.append((a[8], a[9])), real(*a))[1]
        try:
            _x, gamma3, beta3, _r = leaves(True)
            y3 = V.batch_norm_eval(_x.detach(), gamma3, beta3, rm, rv, EPS, True, _r.detach())
            (y3 * dy.reshape(shape).to(DEV)).sum().backward()
        finally:
            ops.batch_norm_eval_backward = real
    assert seen_dx == [(False, True)]
    assert torch.equal(_bits(gamma3.grad), _bits(gamma.grad)) and torch.equal(_bits(beta3.grad), _bits(beta.grad))


# ---- GPU: SurfaceNormalPrediction ----------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_iteration(seeded_weights, frozen_prefix, monkeypatch):
    """One iteration of the SMALL network at B = 2 on the CPU as tests/test_net_autograd_training.py's _sn_oracle_iteration builds it, but WITHOUT
    train_oracle.bn_training(): the oracle's default is eval-mode BatchNorm.  frozen_prefix == "": every BatchNorm frozen, the oracle as it is; else
    oracle.vidc_oracle._bn is replaced for the duration of the call by one that is in training mode unless the BatchNorm's key starts with the prefix."""
    if frozen_prefix not in _ORACLE:
        from oracle import train_oracle as TO
        intr = O.Intrinsics(float(SMALL["fc_img"][0]), float(SMALL["fc_img"][1]), float(SMALL["cc_img"][0]), float(SMALL["cc_img"][1]))
        ins = _inputs(2, 96, 128, 77, 0)
        image, gravity, aligned, normal_gt, mask = ins
        work = {k: (v.detach().clone().requires_grad_(True) if TO.is_parameter(k) else v.detach().clone()) for k, v in seeded_weights["sn"].items()}
        if frozen_prefix:
            def bn(x, sd, p):
                return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                                    training=not p.startswith(frozen_prefix), momentum=0.1, eps=1e-5)
            monkeypatch.setattr(O, "_bn", bn)
        assert not O.BN_TRAINING
        with torch.enable_grad():
            pred = O.surface_normal_forward(work, image, gravity, aligned, intr)
            m = (mask > 0).float()[:, None]
            n = F.normalize(pred, dim=1)
            loss = F.l1_loss(n * m, F.normalize(normal_gt) * m, reduction="sum") / m.sum()
            loss.backward()
        monkeypatch.undo()
        grads = {k: v.grad for k, v in work.items() if v.requires_grad}
        gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
        _ORACLE[frozen_prefix] = {"ins": ins, "intr": intr, "loss": float(loss.detach()), "grad_norm": gn, "grads": grads,
                                  "stats": {k: v for k, v in work.items() if not v.requires_grad}}
    return _ORACLE[frozen_prefix]


def _one_step(cnn, ins):
    image, gravity, aligned, normal_gt, mask = ins
    for p in cnn.parameters():
        p.grad = None
    with torch.enable_grad():
        out = cnn.forward_autograd(image, gravity, aligned)
        loss, _count, _angle = V.normal_l1_loss(out, normal_gt, mask, True)
        loss.backward()
    return loss.detach()


def _check_vs_oracle(tag, cnn, loss, ref):
    """The fp32 bars of tests/test_sn_training.py::test_one_iteration_vs_oracle: loss 1e-5 relative, global gradient norm 1e-3.  The norm of the gradient
    difference and the worst parameter are printed for the record (no bar is set for them there)."""
    gn = _grad_norm(cnn)
    diff2, ref2, worst = 0.0, 0.0, ("", 0.0)
    for n, p in cnn.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
        want = ref["grads"][n].double()
        d2, w2 = float(((p.grad.cpu().double() - want) ** 2).sum()), float((want ** 2).sum())
        diff2, ref2 = diff2 + d2, ref2 + w2
        if w2 > 1e-12 * ref["grad_norm"] ** 2 and (d2 / w2) ** 0.5 > worst[1]:
            worst = (n, (d2 / w2) ** 0.5)
    print("%s: loss %.8f vs %.8f (rel %.2e), grad norm %.6e vs %.6e (rel %.2e), |g - g_ref| / |g_ref| %.2e, worst parameter %s %.2e"
          % (tag, float(loss), ref["loss"], abs(float(loss) - ref["loss"]) / ref["loss"], gn, ref["grad_norm"], abs(gn - ref["grad_norm"]) / gn,
             (diff2 / ref2) ** 0.5, worst[0], worst[1]))
    assert abs(float(loss) - ref["loss"]) < 1e-5 * ref["loss"]
    assert abs(gn - ref["grad_norm"]) < 1e-3 * gn


@gpu
def test_all_frozen_step_vs_eval_mode_oracle_and_round_trip(seeded_weights, monkeypatch):
    """(a) Top module in train(), every BatchNorm2d in eval(): one forward_autograd + loss + backward() leaves running_mean, running_var and
    num_batches_tracked of every BatchNorm bit-unchanged; loss and gradients against the oracle differentiated with eval-mode BatchNorm.
    (e) Then an Adam step and eval(): the inference path runs the updated weights (the oracle on the updated state_dict, tests/test_hip_parity.py's bars for
    this network: max 2e-3, mean 5e-5) and not the output before the step."""
    ref = _oracle_iteration(seeded_weights, "", monkeypatch)
    cnn = _sn_network(seeded_weights, **SMALL)
    ins = [t.to(DEV) for t in ref["ins"]]
    with torch.no_grad():
        before = cnn.eval()(*ins[:3]).cpu()
    cnn.train()
    frozen = _freeze(cnn)
    assert len(frozen) > 100 and cnn.training and not cnn._autograd_dirty
    stats0 = _stat_bits(cnn)
    optimizer = torch.optim.Adam(cnn.parameters(), lr=LR)
    loss = _one_step(cnn, ins)
    assert cnn._autograd_dirty
    stats1 = _stat_bits(cnn)
    changed = [n for n in stats0 if not torch.equal(stats0[n], stats1[n])]
    assert not changed, "frozen BatchNorm statistics were written: %d of %d, first %s" % (len(changed), len(stats0), changed[:3])
    _check_vs_oracle("all frozen", cnn, loss, ref)
    optimizer.step()
    with torch.no_grad():
        after = cnn.eval()(*ins[:3]).cpu()
    assert not cnn._autograd_dirty
    want = O.surface_normal_forward({k: v.detach().cpu() for k, v in cnn.state_dict().items()}, *ref["ins"][:3], ref["intr"])
    d = (after - want).abs()
    print("eval() after the frozen step: max %.3e, mean %.3e vs the oracle" % (float(d.max()), float(d.mean())))
    assert float(d.max()) < 2e-3 and float(d.mean()) < 5e-5
    assert not torch.equal(after, before)


@gpu
def test_frozen_pyramids_training_decoder_vs_mixed_oracle(seeded_weights, monkeypatch):
    """(b) Only resnet_pyramids' BatchNorms in eval(): the pyramid statistics bit-unchanged, every decoder statistic moved and its num_batches_tracked == 1;
    loss and gradients against the oracle whose _bn chooses `training` by key prefix."""
    ref = _oracle_iteration(seeded_weights, "resnet_pyramids.", monkeypatch)
    cnn = _sn_network(seeded_weights, **SMALL).train()
    frozen = _freeze(cnn, "resnet_pyramids.")
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in cnn.modules())
    assert 0 < len(frozen) < n_bn
    stats0 = _stat_bits(cnn)
    loss = _one_step(cnn, [t.to(DEV) for t in ref["ins"]])
    stats1 = _stat_bits(cnn)
    for n in stats0:
        if n.startswith("resnet_pyramids."):
            assert torch.equal(stats0[n], stats1[n]), n
        elif n.endswith("num_batches_tracked"):
            assert int(stats1[n]) == 1, n
        else:
            assert not torch.equal(stats0[n], stats1[n]), n
            want = ref["stats"][n]
            assert float((dict(cnn.named_buffers())[n].cpu() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), n
    _check_vs_oracle("pyramids frozen", cnn, loss, ref)


@gpu
def test_nothing_frozen_is_the_walk_as_it_was(seeded_weights, monkeypatch):
    """(c) With every BatchNorm in train() mode the dispatching Walk.bn gives the loss and gradient bits of a Walk whose bn calls batch_norm_train
    directly (the method as it was before the dispatch)."""
    from vi_depth_completion_amd.networks import autograd_blocks as AB
    ins = [t.to(DEV) for t in _inputs(2, 96, 128, 77, 0)]
    cnn = _sn_network(seeded_weights, **SMALL).train()
    loss_a = _one_step(cnn, ins)
    grads_a = {n: _bits(p.grad).clone() for n, p in cnn.named_parameters()}

    def bn_direct(self, t, m, relu, residual=None):
        self._counters.append(m.num_batches_tracked)
        return self.V.batch_norm_train(t, m.weight, m.bias, m.running_mean, m.running_var, m.momentum, m.eps, relu, residual)[0]

    monkeypatch.setattr(AB.Walk, "bn", bn_direct)
    cnn = _sn_network(seeded_weights, **SMALL).train()
    loss_b = _one_step(cnn, ins)
    assert torch.equal(_bits(loss_a), _bits(loss_b))
    for n, p in cnn.named_parameters():
        assert torch.equal(grads_a[n], _bits(p.grad)), n
    assert all(int(b) == 1 for n, b in cnn.named_buffers() if n.endswith("num_batches_tracked"))


# ---- GPU: SurfaceNormalDORN ----------------------------------------------------------------------------------------------------------------------------
def _dorn_ref_frozen(names, buffers, keeps, mask, gt):
    """tests/test_dorn_autograd_training.py's _dorn_ref with every BatchNorm in eval() mode: F.batch_norm(training=False) on the running statistics."""
    def ref(x, *params):
        P = dict(zip(names, params))
        k1, k2, k3 = [k.to(x.dtype)[:, :, None, None] for k in keeps]

        def bn(t, key, relu=True, res=None):
            y = F.batch_norm(t, buffers[key + ".running_mean"].to(x.dtype), buffers[key + ".running_var"].to(x.dtype), P[key + ".weight"], P[key + ".bias"],
                             training=False, eps=EPS)
            y = y if res is None else y + res
            return F.relu(y) if relu else y

        fe = "feature_extractor."
        t = F.relu(F.conv2d(x, P[fe + "conv1.conv1_1.weight"], stride=2, padding=1))
        t = bn(F.conv2d(t, P[fe + "conv1.conv1_2.weight"], padding=1), fe + "conv1.bn_2")
        t = bn(bn(F.conv2d(t, P[fe + "conv1.conv1_3.weight"], padding=1), fe + "conv1.bn1_3"), fe + "bn1")
        t = F.max_pool2d(t, 3, 2, 1)
        for li, (blocks, stride) in enumerate(zip((3, 4, 23, 3), (1, 2, 1, 1)), start=1):
            for bi in range(blocks):
                p, s = fe + "layer%d.%d." % (li, bi), (stride if bi == 0 else 1)
                u = bn(F.conv2d(t, P[p + "conv1.weight"]), p + "bn1")
                u = bn(F.conv2d(u, P[p + "conv2.weight"], stride=s, padding=1), p + "bn2")
                idn = bn(F.conv2d(t, P[p + "downsample.0.weight"], stride=s), p + "downsample.1", relu=False) if bi == 0 else t
                t = bn(F.conv2d(u, P[p + "conv3.weight"]), p + "bn3", res=idn)
        a = "aspp_module."
        e = F.avg_pool2d(t, 8, 8, (1, 0)) * k1
        e = F.relu(F.linear(e.flatten(1), P[a + "encoder.global_fc.weight"], P[a + "encoder.global_fc.bias"]))
        e = F.conv2d(e[:, :, None, None], P[a + "encoder.conv1.weight"], P[a + "encoder.conv1.bias"])
        branches = [F.interpolate(e, size=(30, 40), mode="bilinear", align_corners=True)]
        for name, d in (("aspp1", 0), ("aspp2", 6), ("aspp3", 12), ("aspp4", 18)):
            q = a + name
            u = bn(F.conv2d(t, P[q + ".0.weight"], P[q + ".0.bias"], padding=d, dilation=max(d, 1)), q + ".1")
            branches.append(bn(F.conv2d(u, P[q + ".3.weight"], P[q + ".3.bias"]), q + ".4"))
        h = F.relu(F.conv2d(torch.cat(branches, dim=1) * k2, P[a + "concat_process.1.weight"], P[a + "concat_process.1.bias"])) * k3
        y = F.interpolate(F.conv2d(h, P[a + "concat_process.4.weight"], P[a + "concat_process.4.bias"]), size=(240, 320), mode="bilinear", align_corners=True)
        return _masked_l1(F.normalize(y, dim=1), gt, mask), None
    return ref


@gpu
def test_dorn_all_frozen_matches_float64_restatement():
    """(d) SurfaceNormalDORN with seeded weights, B = 1 at 240 x 320, every BatchNorm frozen, the dropout seed fixed (the keep tables of seed 777): every
    parameter's gradient of the masked L1 loss against the float64 restatement with F.batch_norm(training=False), at the bars of
    tests/test_dorn_autograd_training.py (tests/test_torch_ops_autograd.py's _compare, "l1": 4 x the float32 CPU restatement's own deviation); no BatchNorm
    statistic is written by any of the passes."""
    from torch.nn.utils import stateless
    from vi_depth_completion_amd.networks.surface_normal_dorn import SurfaceNormalDORN
    weights, x, mask, gt = _dorn_case()
    cnn = SurfaceNormalDORN(pretrained=False).to(DEV)
    cnn.load_state_dict(weights)
    cnn.train()
    assert len(_freeze(cnn)) > 100
    mask_d, gt_d = mask.to(DEV), gt.to(DEV)
    probe = torch.zeros(1, 1, 1, 2560, device=DEV)
    keeps = [V.dropout2d(probe[..., :c], 0.5, 777, layer)[1] for layer, c in enumerate((2048, 2560, 2048))]
    names = [n for n, _ in cnn.named_parameters()]
    buffers = {n: b.detach().cpu().clone() for n, b in cnn.named_buffers()}
    stats0 = _stat_bits(cnn)

    def ours(x_, *params):
        with stateless._reparametrize_module(cnn, dict(zip(names, params))):
            return V.normal_l1_loss(cnn.forward_autograd(x_, dropout_seed=777, _keeps=keeps), gt_d, mask_d, False)[0]

    tensors = [x] + [weights[n] for n in names]
    _compare("dorn-frozen", _dorn_ref_frozen(names, buffers, [k.cpu() for k in keeps], mask, gt), ours, tensors, ["x"] + names, how="l1")
    stats1 = _stat_bits(cnn)
    assert all(torch.equal(stats0[n], stats1[n]) for n in stats0)
