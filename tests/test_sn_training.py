"""Training step of the surface-normal network: the normal loss kernel against the reference's own record
(tests/golden/normal_loss.npz, tools/make_golden_normal_loss.py) and against float64 torch autograd, the three-channel head backward
against float64 autograd, one whole iteration of `SurfaceNormalTrainer` against the CPU oracle, graph replay against eager steps, a short
run that learns, and the refusals.  Tolerances are stated per test."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vi_depth_completion_amd import synthetic as S

gpu = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(output_size=(96, 128), fc_img=np.array([81.0, 81.0]), cc_img=np.array([63.9, 47.9]))      # W = ceil(2 cx) = 128, H = ceil(2 cy) = 96


# ---- the loss kernel ------------------------------------------------------------------------------------------------------------------
def _normal_loss(pred, normal_gt, mask, flag, stream=None):
    """vidc_normal_l1_loss on CPU inputs -> (loss, N, angle, dpred) on the CPU."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, _, H, W = pred.shape
    p, g, m = pred.float().contiguous().to(DEV), normal_gt.float().contiguous().to(DEV), mask.float().contiguous().to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        st = torch.zeros(3, dtype=torch.float64, device=DEV)
        dp = torch.full((B, 3, H, W), 7.0, device=DEV)
        sc = torch.empty(lib.vidc_normal_l1_loss_scratch_bytes(B, H, W), dtype=torch.uint8, device=DEV)
        L.check(lib.vidc_normal_l1_loss(L.ptr(p), L.ptr(g), L.ptr(m), B, H, W, int(flag), L.ptr(st), L.ptr(st[1:]), L.ptr(st[2:]), L.ptr(dp), L.ptr(sc),
                                        L.current_stream()), "normal loss")
    torch.cuda.synchronize()
    st = st.cpu()
    return float(st[0]), float(st[1]), float(st[2]), dp.cpu()


@gpu
@pytest.mark.parametrize("flag,tag", [(False, "raw"), (True, "norm")])
def test_normal_loss_kernel_vs_the_references_record(golden_dir, flag, tag):
    """The reference's compute_normal_vectors_loss_l1 on (2, 3, 12, 16) inputs, as shipped (normalize_prediction=False) and with the one
    undefined name read as F.normalize (True).  loss 1e-6 relative; angle 1e-4 relative: the record is fp32 torch, the generator kept
    |n . gh| <= 0.999, where acos amplifies a 2e-7 dot error to under 5e-6 rad per pixel, the rest is fp32 summation -- a 10x margin;
    dpred within 2e-4 of max |want| (the fp32 kernel bar), no element excluded: the generator left no sign ties."""
    f = np.load(os.path.join(golden_dir, "normal_loss.npz"))
    pred, gt, mask = (torch.from_numpy(f[k]) for k in ("pred", "normal_gt", "mask"))
    loss, n, angle, dp = _normal_loss(pred, gt, mask, flag)
    want = torch.from_numpy(f["dpred_" + tag])
    err = float((dp - want).abs().max())
    print("loss %.8f vs %.8f, angle %.4f vs %.4f, N %d, dpred max|diff| %.3e of %.3e" % (loss, float(f["loss_" + tag]), angle, float(f["angle_" + tag]), n, err,
                                                                                       float(want.abs().max())))
    assert n == float((mask > 0).sum())
    assert abs(loss - float(f["loss_" + tag])) <= 1e-6 * float(f["loss_" + tag])
    assert abs(angle - float(f["angle_" + tag])) <= 1e-4 * float(f["angle_" + tag])
    assert err <= 2e-4 * float(want.abs().max())


def _loss_case(B, H, W, exact_row, zero_row):
    g = torch.Generator().manual_seed(11)
    pred = torch.randn(B, 3, H, W, generator=g) * (0.3 + 2.0 * torch.rand(B, 1, H, W, generator=g))
    gt = torch.randn(B, 3, H, W, generator=g) * (0.3 + 2.0 * torch.rand(B, 1, H, W, generator=g))
    on = torch.rand(B, H, W, generator=g) < 0.7
    pick = torch.rand(B, H, W, generator=g)
    mask = torch.where(on, torch.where(pick < 0.3, torch.tensor(0.5), torch.where(pick < 0.6, torch.tensor(2.0), torch.tensor(1.0))),
                       torch.where(pick < 0.5, torch.tensor(0.0), torch.tensor(-1.0)))
    unit = torch.tensor([0.0, 0.0, 1.0]).view(1, 3, 1)
    pred[:, :, exact_row, :] = unit                  # prediction == ground truth == (0, 0, 1) exactly: term 0, gradient 0, angle 0
    gt[:, :, exact_row, :] = unit
    mask[:, exact_row, :] = 1.0
    pred[:, :, zero_row, :] = 0.0                    # the zeros the inverse warp leaves outside the warped region; half of them counted
    mask[:, zero_row, : W // 2] = 1.0
    mask[:, zero_row, W // 2:] = 0.0
    kind = torch.zeros(B, H, W, dtype=torch.long)    # 0 regular, 1 exact match, 2 zero vector
    kind[:, exact_row, :] = 1
    kind[:, zero_row, :] = 2
    return pred, gt, mask, kind


@gpu
@pytest.mark.parametrize("B,H,W", [(2, 15, 20), (1, 7, 9)])
@pytest.mark.parametrize("flag", [False, True])
def test_normal_loss_kernel_vs_float64_autograd(B, H, W, flag):
    """Seeded inputs of non-unit length, about 30 % masked out, a band where prediction and ground truth are (0, 0, 1) exactly and a band
    of zero predictions.  (2, 15, 20): 300 pixels per image, not a multiple of the workgroup, four pixels per thread; (1, 7, 9): 63 pixels,
    the one-pixel-per-thread form.  The reference restated in float64 torch; loss and angle 1e-6 relative (fp64 on both sides).  dpred per
    class of pixel -- the gradient at the zero vectors is g / 1e-12 and would otherwise set the scale -- each class within 2e-4 of its own
    max |want|; elements with |n_c - gh_c| < 1e-6 (a sign that fp32 inputs do not decide) may be left out of the regular class, at most
    0.1 % of the unmasked elements.  The same call on another stream: identical bits.  Mask values 0.5 and 2.0 count as 1, negative as 0."""
    pred, gt, mask, kind = _loss_case(B, H, W, 1, 3)
    p = pred.double().requires_grad_(True)
    m = (mask > 0).double()[:, None]
    with torch.enable_grad():
        gh = F.normalize(gt.double(), dim=1, eps=1e-12)
        n = F.normalize(p, dim=1, eps=1e-12) if flag else p
        loss_w = (n * m - gh * m).abs().sum() / m.sum()
        angle_w = (torch.acos(torch.clamp((n * gh).sum(1, keepdim=True), -1, 1)) / np.pi * 180 * m).sum()
        loss_w.backward()
    want, loss_w, angle_w = p.grad, loss_w.detach(), angle_w.detach()
    loss, cnt, angle, dp = _normal_loss(pred, gt, mask, flag)
    print("loss %.10f vs %.10f, angle %.6f vs %.6f" % (loss, float(loss_w), angle, float(angle_w)))
    assert cnt == float(m.sum())
    assert abs(loss - float(loss_w)) <= 1e-6 * float(loss_w)
    assert abs(angle - float(angle_w)) <= 1e-6 * float(angle_w)
    on3 = (m > 0).expand(B, 3, H, W)
    tie = ((n.detach() - gh).abs() < 1e-6) & on3 & (kind[:, None] == 0)
    assert int(tie.sum()) <= 1e-3 * int(on3.sum())
    assert torch.equal(dp[~on3], torch.zeros_like(dp[~on3]))
    for k, name in enumerate(("regular", "exact match", "zero vector")):
        sel = (kind[:, None] == k).expand(B, 3, H, W) & ~tie
        err, scale = float((dp.double() - want)[sel].abs().max()), float(want[sel].abs().max())
        print("dpred %s: max|diff| %.3e, max|want| %.3e" % (name, err, scale))
        assert err <= 2e-4 * scale, name
    assert float(want[(kind[:, None] == 1).expand(B, 3, H, W)].abs().max()) == 0.0
    if flag:
        assert float(want[(kind[:, None] == 2).expand(B, 3, H, W)].abs().max()) > 1e8      # g / eps / N
    again = _normal_loss(pred, gt, mask, flag, stream=torch.cuda.Stream())
    assert (loss, cnt, angle) == again[:3] and torch.equal(dp.view(torch.int32), again[3].view(torch.int32))
    binary = _normal_loss(pred, gt, (mask > 0).float(), flag)
    assert (loss, cnt, angle) == binary[:3] and torch.equal(dp.view(torch.int32), binary[3].view(torch.int32))


# ---- the head backward ----------------------------------------------------------------------------------------------------------------
def _head_backward_multi(g_low, x, wgt, pad, ld=None):
    """vidc_head_backward_multi on CPU inputs -> (dx, dw, dbias) on the CPU.  ld: x and dx are channels 2 .. 2 + C of buffers ld wide; what
    the kernel leaves of dx's buffer outside the slice must be the fill."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, h, w, C = x.shape
    co = wgt.shape[0]
    ld = C if ld is None else ld
    off = 2 if ld > C else 0
    gd, wd = g_low.to(DEV), wgt.to(DEV)
    x_buf, dx_buf = torch.full((B, h, w, ld), 3.0, device=DEV), torch.full((B, h, w, ld), 7.0, device=DEV)
    xd, dx = x_buf[..., off:off + C], dx_buf[..., off:off + C]
    xd.copy_(x)
    dw, db = torch.full((co, C), 7.0, device=DEV), torch.full((co,), 7.0, device=DEV)
    sc = torch.empty(lib.vidc_head_backward_multi_scratch_bytes(B, h, w, C, co, pad), dtype=torch.uint8, device=DEV)
    L.check(lib.vidc_head_backward_multi(L.ptr(gd), L.ptr(xd), L.ptr(wd), L.ptr(dx), L.ptr(dw), L.ptr(db), B, h, w, C, ld, ld, co, pad, L.ptr(sc), L.current_stream()),
            "head_backward_multi")
    torch.cuda.synchronize()
    outside = torch.cat([dx_buf[..., :off], dx_buf[..., off + C:]], -1)
    assert torch.equal(outside, torch.full_like(outside, 7.0))
    return dx.cpu().contiguous(), dw.cpu(), db.cpu()


def _within(got, want, name):
    err, scale = float((got.double() - want.double()).abs().max()), float(want.abs().max())
    print("%s: max|diff| %.3e, max|want| %.3e" % (name, err, scale))
    assert err <= 2e-4 * scale, name


def _head_case(B, h, w, C, co, pad, seed):
    """Seeded (g_low, x, wgt) and Conv2d(C, co, 1, padding=pad) differentiated by float64 F.conv2d autograd: (dx NHWC, dw, dbias)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g)
    wgt, bias = torch.randn(co, C, generator=g) * 0.2, torch.randn(co, generator=g)
    g_low = torch.randn(B * co, h + 2 * pad, w + 2 * pad, generator=g)
    xr, wr, br = x.double().permute(0, 3, 1, 2).requires_grad_(True), wgt.double().requires_grad_(True), bias.double().requires_grad_(True)
    with torch.enable_grad():
        y = F.conv2d(xr, wr[:, :, None, None], br, padding=pad)
        (y * g_low.double().view(B, co, h + 2 * pad, w + 2 * pad)).sum().backward()
    return (g_low, x, wgt), (xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad)


def _check_head_backward_multi(B, h, w, C, co, pad, ld=None):
    ins, want = _head_case(B, h, w, C, co, pad, 5)
    got = _head_backward_multi(*ins, pad, ld)
    for a, b, name in zip(got, want, ("dx", "dw", "dbias")):
        _within(a, b, name)
    for a, b in zip(got, _head_backward_multi(*ins, pad, ld)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@gpu
@pytest.mark.parametrize("h,w,pad", [(5, 7, 0), (5, 7, 1), (13, 21, 0), (45, 50, 1)])
def test_head_backward_multi_vs_float64_autograd(h, w, pad):
    """Conv2d(64, 3, 1, padding=pad) differentiated: dx, dw, dbias against float64 F.conv2d autograd within 2e-4 of max |want|, identical
    bits on a second run.  5 x 7 is one chunk of the weight-gradient reduction, 13 x 21 three, 45 x 50 eighteen and two workgroups of the
    bias sum."""
    _check_head_backward_multi(2, h, w, 64, 3, pad)


@gpu
@pytest.mark.parametrize("B,h,w,C,co,pad,ld", [(2, 65, 64, 64, 3, 1, None), (2, 5, 7, 20, 3, 0, None), (2, 13, 21, 64, 3, 1, 68), (1, 6, 5, 20, 4, 0, 24)],
                         ids=["33-chunks", "60-outputs", "ld-68", "cout-4-ld-24"])
def test_head_backward_multi_vs_float64_autograd_edge_geometries(B, h, w, C, co, pad, ld):
    """The same check (same bar, same second run) where the geometry takes another path.  2 x 65 x 64 rows = 8320 = 33 chunks of 256: a lane
    of the final reduction (32 lanes) sums more than one chunk.  C = 20, Cout = 3: 60 outputs, not a multiple of the 8 outputs a workgroup
    of the final reduction holds, and fewer channels than a workgroup has threads.  ld = C + 4: x and dx are channel slices of wider
    buffers, whose other channels the kernels must leave alone -- once more with the largest Cout the entry takes."""
    _check_head_backward_multi(B, h, w, C, co, pad, ld)


@gpu
def test_head_backward_one_channel_vs_float64_autograd():
    """vidc_head_backward (the depth network's head: Conv2d(C, 1, 1, padding=1)) against float64 F.conv2d autograd within 2e-4 of max
    |want| (the bar of the tests above); it forwards to vidc_head_backward_multi with Cout = 1, pad = 1, so its bits are that call's, and
    those of a second run.  2 x 13 x 21 rows: three chunks."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, h, w, C = 2, 13, 21, 64
    (g_low, x, wgt), want = _head_case(B, h, w, C, 1, 1, 6)
    assert lib.vidc_head_backward_scratch_bytes(B, h, w, C) == lib.vidc_head_backward_multi_scratch_bytes(B, h, w, C, 1, 1)

    def run():
        gd, xd, wd = g_low.to(DEV), x.to(DEV), wgt.to(DEV)
        dx, dw, db = torch.full((B, h, w, C), 7.0, device=DEV), torch.full((1, C), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
        sc = torch.empty(lib.vidc_head_backward_scratch_bytes(B, h, w, C), dtype=torch.uint8, device=DEV)
        L.check(lib.vidc_head_backward(L.ptr(gd), L.ptr(xd), L.ptr(wd), L.ptr(dx), L.ptr(dw), L.ptr(db), B, h, w, C, C, C, L.ptr(sc), L.current_stream()), "head_backward")
        torch.cuda.synchronize()
        return dx.cpu(), dw.cpu(), db.cpu()

    got = run()
    for a, b, name in zip(got, want, ("dx", "dw", "dbias")):
        _within(a, b, name)
    for other in (_head_backward_multi(g_low, x, wgt, 1), run()):
        for a, b in zip(got, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _network(seeded_weights, **kw):
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    cnn = SurfaceNormalPrediction(**kw).to(DEV)
    st = cnn.state_dict()
    st.update({k: v.to(DEV) for k, v in seeded_weights["sn"].items()})
    cnn.load_state_dict(st)
    return cnn.train()


def _inputs(B, H, W, seed, frame0):
    b = S.synthetic_batch(B, H, W, seed, frame0=frame0)
    normal_gt = S.normal01(seed, "sn.gt.%d" % frame0, (B, 3, H, W)).float() * 1.7
    mask = (S.uniform01(seed, "sn.mask.%d" % frame0, (B, H, W)) < 0.7).float()
    return b["image"], b["gravity"], b["aligned_direction"], normal_gt, mask


LR = 1e-4
PROBES = ("feature_concat.2.weight", "feature_concat.0.bias")
STATS = ("resnet_pyramids.conv1.bn_2.running_var", "feature4_upsamping.1.running_mean")


@pytest.fixture(scope="module")
def oracle_iteration(seeded_weights):
    """One iteration on the CPU, shared by the precisions: oracle.vidc_oracle.surface_normal_forward under train-mode BatchNorm with the
    parameters as leaves (as oracle.train_oracle.forward_backward does for the depth network), the loss of network_run.py:182-189 /
    normal_utils.py:20-34 restated (`Normalize` read as F.normalize), backward, oracle.train_oracle.adam_step."""
    from oracle import train_oracle as T
    from oracle import vidc_oracle as O
    intr = O.Intrinsics(0.5 * 577.87061, 0.5 * 580.25851, 0.5 * 319.87654, 0.5 * 239.87603)      # SurfaceNormalPrediction's default fc_img / cc_img
    assert (intr.H, intr.W) == (240, 320)
    ins = _inputs(1, 240, 320, 1234, 3)
    image, gravity, aligned, normal_gt, mask = ins
    sd = seeded_weights["sn"]
    work = {}
    for k, v in sd.items():
        work[k] = v.detach().clone().requires_grad_(True) if T.is_parameter(k) else v.detach().clone()
    with torch.enable_grad(), T.bn_training():
        pred = O.surface_normal_forward(work, image, gravity, aligned, intr)
        m = (mask > 0).float()[:, None]
        gh = F.normalize(normal_gt)
        n = F.normalize(pred, dim=1)
        loss = F.l1_loss(n * m, gh * m, reduction="sum") / m.sum()
        angle = (torch.acos(torch.clamp((n * gh).sum(1, keepdim=True), -1, 1)) / np.pi * 180 * m).sum()
        loss.backward()
    params = {k: v.detach() for k, v in work.items() if v.requires_grad}
    grads = {k: work[k].grad for k in params}
    new = T.adam_step(params, grads, {}, LR)
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    return {"ins": ins, "loss": float(loss.detach()), "angle": float(angle.detach()), "grad_norm": gn, "new": {k: new[k] for k in PROBES}, "stats": {k: work[k] for k in STATS}}


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_one_iteration_vs_oracle(oracle_iteration, seeded_weights, monkeypatch, precision):
    """One `_run_training_iteration` of the 240 x 320 network on one frame against the CPU oracle, with the bars tests/test_training.py sets
    for the same quantities of the depth network: loss 1e-5 relative (2e-5 in bf16x3, that file's bar for both modes), global gradient
    norm 1e-3, the two probed parameters within 2.1 lr after the Adam step (a sign flip of a near-zero gradient moves a value by 2 lr), one
    pyramid and one decoder running statistic within 1e-4 max(1, |ref|), num_batches_tracked == 1.  The angle sum (logged, not a bar of
    that file) within 1e-3 relative."""
    from vi_depth_completion_amd.training import SurfaceNormalTrainer
    monkeypatch.setenv("VIDC_TRAIN_PRECISION", precision)
    ref = oracle_iteration
    cnn = _network(seeded_weights)
    tr = SurfaceNormalTrainer(cnn, LR)
    assert tr.layout == "per_pyramid" and not tr.grouped
    loss = float(tr.step(*[t.to(DEV) for t in ref["ins"]]))
    torch.cuda.synchronize()
    gn = float(torch.sqrt((tr.flat_g.double() ** 2).sum()))
    print("loss %.8f vs %.8f, angle %.3f vs %.3f, grad norm %.6e vs %.6e" % (loss, ref["loss"], float(tr.last_angle), ref["angle"], gn, ref["grad_norm"]))
    assert abs(loss - ref["loss"]) < (1e-5 if precision == "fp32" else 2e-5) * ref["loss"]
    assert abs(gn - ref["grad_norm"]) < 1e-3 * gn
    assert abs(float(tr.last_angle) - ref["angle"]) < 1e-3 * ref["angle"]
    assert float(tr.last_count) == float((ref["ins"][4] > 0).sum())
    sd = cnn.state_dict()
    for k in PROBES:
        err = float((sd[k].cpu() - ref["new"][k]).abs().max())
        print("%s after the step: max|diff| %.3e (lr %.0e)" % (k, err, LR))
        assert err < 2.1 * LR, k
    for k in STATS:
        want = ref["stats"][k]
        assert float((sd[k].cpu() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), k
    assert int(sd["resnet_pyramids.bn1.num_batches_tracked"]) == 1


@gpu
def test_graph_replay_equals_eager_steps(seeded_weights, monkeypatch):
    """Five steps of a 96 x 128 network on changing two-frame batches, VIDC_TRAIN_GRAPH=1 against 0: the same kernels with fixed-order
    reductions, so losses, angle sums and every parameter and buffer are bit-identical; with the graph on, steps three to five replay ONE
    captured graph."""
    from vi_depth_completion_amd.training import SurfaceNormalTrainer
    runs = []
    for use_graph in ("0", "1"):
        monkeypatch.setenv("VIDC_TRAIN_GRAPH", use_graph)
        cnn = _network(seeded_weights, **SMALL)
        tr = SurfaceNormalTrainer(cnn, 1e-4)
        assert tr.use_graph == (use_graph == "1")
        losses, angles = [], []
        for it in range(5):
            losses.append(float(tr.step(*[t.to(DEV) for t in _inputs(2, 96, 128, 77, 2 * it)])))
            angles.append(float(tr.last_angle))
        assert len(tr._graphs) == (1 if use_graph == "1" else 0)
        runs.append((losses, angles, {k: v.clone() for k, v in cnn.state_dict().items()}))
    (l0, a0, s0), (l1, a1, s1) = runs
    print("losses", l0, "angles", a0)
    assert all(np.isfinite(l0)) and l0 == l1 and a0 == a1
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    assert int(s1["resnet_pyramids.bn1.num_batches_tracked"]) == 5


@gpu
def test_it_learns_in_plain_bf16(seeded_weights, monkeypatch):
    """VIDC_TRAIN_PRECISION=bf16, a fixed batch, 8 steps at lr = 1e-3: the last loss is under 0.9 x the first (the bar of
    test_plain_bf16_training_mode), and the stepped network serves inference again with other normals than before (`_invalidate`)."""
    from vi_depth_completion_amd.training import SurfaceNormalTrainer
    monkeypatch.setenv("VIDC_TRAIN_PRECISION", "bf16")
    cnn = _network(seeded_weights, **SMALL)
    image, gravity, aligned, _gt, mask = [t.to(DEV) for t in _inputs(2, 96, 128, 77, 0)]
    normal_gt = F.normalize(torch.stack([0.4 * (image[:, 0] - 0.5), -0.6 + 0.2 * (image[:, 1] - 0.5), -0.7 + 0.0 * image[:, 2]], dim=1), dim=1) * 2.0
    cnn.eval()
    before = cnn(image, gravity, aligned)
    cnn.train()
    tr = SurfaceNormalTrainer(cnn, 1e-3)
    losses = [float(tr.step(image, gravity, aligned, normal_gt, mask)) for _ in range(8)]
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0]
    cnn.eval()
    after = cnn(image, gravity, aligned)
    assert torch.isfinite(after).all() and float((after - before).abs().mean()) > 1e-4


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refuses_use_mask_networks_and_process_groups(monkeypatch):
    from vi_depth_completion_amd import sharding
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.training import SurfaceNormalTrainer
    with pytest.raises(RuntimeError, match="use_mask"):
        SurfaceNormalTrainer(SurfaceNormalPrediction(use_mask=True).train())
    cnn = SurfaceNormalPrediction().train()
    monkeypatch.setattr(sharding, "collectives_active", lambda: True)      # what an initialised two-rank group answers
    with pytest.raises(RuntimeError, match="one rank"):
        SurfaceNormalTrainer(cnn)


def test_train_mode_forward_names_the_trainer():
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    cnn = SurfaceNormalPrediction().train()
    with pytest.raises(RuntimeError, match="SurfaceNormalTrainer"):
        cnn(torch.zeros(1, 3, 240, 320), torch.zeros(1, 3), torch.zeros(1, 3))


@gpu
def test_refuses_eval_networks_cpu_tensors_and_late_process_groups(seeded_weights, monkeypatch):
    from vi_depth_completion_amd import sharding
    from vi_depth_completion_amd.training import SurfaceNormalTrainer
    cnn = _network(seeded_weights, **SMALL)
    tr = SurfaceNormalTrainer(cnn, 1e-4)
    ins = _inputs(1, 96, 128, 77, 0)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        tr.step(*ins)
    cnn.eval()
    with pytest.raises(RuntimeError, match=r"cnn\.train\(\)"):
        tr.step(*[t.to(DEV) for t in ins])
    cnn.train()
    monkeypatch.setattr(sharding, "collectives_active", lambda: True)
    with pytest.raises(RuntimeError, match="one rank"):
        tr.step(*[t.to(DEV) for t in ins])
