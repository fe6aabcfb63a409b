"""The Cin = 64 form of the one-launch Winograd F(4x4, 3x3) kernel (csrc/wfused.hip, tile VIDC_TILE_WINO4_FUSED): persistent workgroups that walk
items of 16 tiles x 64 output channels, the input transform of a tile block computed once for all of them (the 64-channel stem convs conv1_2 / conv1_3,
torchvision-style deep stem as used at networks/surface_normal.py).  The smallest shapes at which it can go wrong: one partial block of 16 tiles; full
blocks plus a partial one, blocks across image boundaries, both 64-channel halves of Cout = 128; a partial tile row and column.  Against F.conv2d in
float64 and the three-launch path with the tolerances of tests/test_wfused.py; bits independent of the groups in the launch, the batch partners and the
workgroup cap; which shapes the launcher gives to which form; what the engine records."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vi_depth_completion_amd import synthetic as S

DEV = "cuda"
gpu = pytest.mark.gpu

# B, H, W, cout, G (Cin = 64)
CASES = {"a": (1, 8, 12, 64, 1),       # 6 tiles: one partial block of 16
         "b": (3, 12, 20, 128, 4),     # 45 tiles per group: two full blocks and a partial one, blocks across image boundaries, both Cout halves
         "c": (2, 6, 10, 64, 3)}       # partial tile row and column (edge masks with m = 4)
CIN = 64


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _case(name, cin=CIN):
    """Inputs and the float64 conv + affine of a case (computed once, shared, never modified)."""
    B, H, W, cout, G = CASES[name]
    seed = 60 + ord(name)
    x = S.normal01(seed, "x", (B, G * cin, H, W)).float()
    w = [S.normal01(seed, "w%d" % g, (cout, cin, 3, 3), scale=float(np.sqrt(2.0 / (cin * 9)))).float() for g in range(G)]
    s1 = S.uniform01(seed, "s1", (G, cout)) + 0.5
    b1 = S.normal01(seed, "b1", (G, cout)).float() * 0.1
    outs = [F.conv2d(x[:, g * cin:(g + 1) * cin].double(), w[g].double(), None, 1, 1) * s1[g].double().view(1, -1, 1, 1) + b1[g].double().view(1, -1, 1, 1) for g in range(G)]
    return x, w, s1, b1, torch.cat(outs, 1)


def _stem(monkeypatch, cap=None):
    """The launcher gives every qualifying shape to the Cin = 64 form (its threshold is far above these tile counts) and reports the form it chose."""
    monkeypatch.setenv("VIDC_WFUSED_STEM_MIN_TILES", "1")
    monkeypatch.setenv("VIDC_WFUSED_TRACE", "1")
    if cap is None:
        monkeypatch.delenv("VIDC_WFUSED_STEM_CAP", raising=False)
    else:
        monkeypatch.setenv("VIDC_WFUSED_STEM_CAP", str(cap))


def _forms(capfd):
    return [line.split()[2] for line in capfd.readouterr().err.splitlines() if line.startswith("wino4f: form")]


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_stem_form_vs_float64_and_three_launch_path(name, monkeypatch, capfd):
    from vi_depth_completion_amd import ops
    x, w, s1, b1, conv = _case(name)
    ref = F.relu(conv)
    xd, wd = nhwc(x).to(DEV), [t.to(DEV) for t in w]
    _stem(monkeypatch)
    capfd.readouterr()
    y = ops.conv3x3_winograd_fused(xd, wd, s1.to(DEV), b1.to(DEV), relu1=True)
    torch.cuda.synchronize()
    assert _forms(capfd) == ["stem"]
    err = (nchw(y).cpu().double() - ref).abs().max().item()
    y3 = ops.conv3x3_winograd(xd, wd, s1.to(DEV), b1.to(DEV), 4, relu1=True)
    d3 = (y - y3).abs().max().item()
    e3 = (nchw(y3).cpu().double() - ref).abs().max().item()
    print("case %s: max|stem - float64| %.3e, max|stem - three launches| %.3e, max|three launches - float64| %.3e" % (name, err, d3, e3))
    assert err < 2e-4, err
    assert d3 < 2e-4, d3
    assert err < 5.0 * e3 + 1e-6, (err, e3)


@gpu
def test_second_affine_and_no_relu(monkeypatch, capfd):
    from vi_depth_completion_amd import ops
    x, w, s1, b1, conv = _case("c")
    G, cout = CASES["c"][4], CASES["c"][3]
    s2 = S.uniform01(71, "s2", (G, cout)) + 0.5
    b2 = S.normal01(71, "b2", (G, cout)).float() * 0.1
    xd, wd = nhwc(x).to(DEV), [t.to(DEV) for t in w]
    ref2 = F.relu(F.relu(conv) * s2.double().view(1, -1, 1, 1) + b2.double().view(1, -1, 1, 1))
    _stem(monkeypatch)
    capfd.readouterr()
    y = ops.conv3x3_winograd_fused(xd, wd, s1.to(DEV), b1.to(DEV), relu1=True, scale2=s2.to(DEV), shift2=b2.to(DEV), relu2=True)
    assert (nchw(y).cpu().double() - ref2).abs().max().item() < 2e-4
    y3 = ops.conv3x3_winograd(xd, wd, s1.to(DEV), b1.to(DEV), 4, relu1=True, scale2=s2.to(DEV), shift2=b2.to(DEV), relu2=True)
    assert (y - y3).abs().max().item() < 2e-4
    y = ops.conv3x3_winograd_fused(xd, wd, s1.to(DEV), b1.to(DEV))
    assert (nchw(y).cpu().double() - conv).abs().max().item() < 2e-4
    assert bool((y < 0).any())
    y = ops.conv3x3_winograd_fused(xd, wd, s1.to(DEV), b1.to(DEV), scale2=s2.to(DEV), shift2=b2.to(DEV))      # AFFINE2 without either ReLU
    assert (nchw(y).cpu().double() - (conv * s2.double().view(1, -1, 1, 1) + b2.double().view(1, -1, 1, 1))).abs().max().item() < 2e-4
    assert _forms(capfd) == ["stem"] * 3


@gpu
def test_bits_do_not_depend_on_groups_batch_partners_or_the_workgroup_cap(monkeypatch, capfd):
    from vi_depth_completion_amd import ops
    x, w, s1, b1, _conv = _case("b")
    B, _H, _W, cout, G = CASES["b"]
    xd, wd, s1d, b1d = nhwc(x).to(DEV), [t.to(DEV) for t in w], s1.to(DEV), b1.to(DEV)
    _stem(monkeypatch)
    capfd.readouterr()
    full = ops.conv3x3_winograd_fused(xd, wd, s1d, b1d, relu1=True)          # 3 tile blocks x 4 groups x 2 halves = 24 items, one per workgroup
    # the same groups launched singly, and a three-group subset (the head / tail ticks of a stream)
    for g in range(G):
        one = ops.conv3x3_winograd_fused(xd[..., g * CIN:(g + 1) * CIN].contiguous(), wd[g:g + 1], s1d[g:g + 1], b1d[g:g + 1], relu1=True)
        assert torch.equal(one, full[..., g * cout:(g + 1) * cout]), g
    part = ops.conv3x3_winograd_fused(xd[..., CIN:].contiguous(), wd[1:], s1d[1:], b1d[1:], relu1=True)
    assert torch.equal(part, full[..., cout:])
    # a frame alone: other tile blocks (its tiles start a block of their own), other items, other workgroups
    for b in range(B):
        alone = ops.conv3x3_winograd_fused(xd[b:b + 1].contiguous(), wd, s1d, b1d, relu1=True)
        assert torch.equal(alone[0], full[b]), b
    assert _forms(capfd) == ["stem"] * (2 + G + B)
    # the workgroup cap: one workgroup walks all 24 items; three walk eight each
    for cap in (1, 3):
        _stem(monkeypatch, cap)
        assert torch.equal(ops.conv3x3_winograd_fused(xd, wd, s1d, b1d, relu1=True), full), cap
    # ... and the other form of the tile computes every output element in the same order
    monkeypatch.setenv("VIDC_WFUSED_STEM_MIN_TILES", "0")
    capfd.readouterr()
    form4 = ops.conv3x3_winograd_fused(xd, wd, s1d, b1d, relu1=True)
    assert _forms(capfd) == ["4"]
    assert torch.equal(form4, full)


@gpu
def test_dispatch(monkeypatch, capfd):
    """Cin = 64 below the launcher's own threshold, and Cin != 64 whatever the threshold, run the form they ran before."""
    from vi_depth_completion_amd import ops
    x, w, s1, b1, conv = _case("a")
    xd, wd = nhwc(x).to(DEV), [t.to(DEV) for t in w]
    monkeypatch.delenv("VIDC_WFUSED_STEM_MIN_TILES", raising=False)
    monkeypatch.delenv("VIDC_WFUSED_STEM_CAP", raising=False)
    monkeypatch.setenv("VIDC_WFUSED_TRACE", "1")
    capfd.readouterr()
    y = ops.conv3x3_winograd_fused(xd, wd, s1.to(DEV), b1.to(DEV), relu1=True)
    assert _forms(capfd) == ["4"]
    assert (nchw(y).cpu().double() - F.relu(conv)).abs().max().item() < 2e-4
    _stem(monkeypatch)
    for cin, cout in ((32, 64), (128, 64), (64, 96)):          # not 64 input channels; no whole 64-channel blocks of output
        xs = S.normal01(81, "x", (1, cin, 8, 12)).float()
        ws = [S.normal01(81, "w", (cout, cin, 3, 3), scale=float(np.sqrt(2.0 / (cin * 9)))).float()]
        one, zero = torch.ones(1, cout), torch.zeros(1, cout)
        y = ops.conv3x3_winograd_fused(nhwc(xs).to(DEV), [ws[0].to(DEV)], one.to(DEV), zero.to(DEV))
        assert _forms(capfd) == ["4"], (cin, cout)
        assert (nchw(y).cpu().double() - F.conv2d(xs.double(), ws[0].double(), None, 1, 1)).abs().max().item() < 2e-4, (cin, cout)


STEM_KEYS = ("W:M81920_N64_K576_k3s1_G4", "W:M81920_N128_K576_k3s1_G4")


def test_engine_records_the_stem_layers_on_the_fused_tile_where_the_table_says_5(monkeypatch):
    """CPU dry-run recording (no HIP call): with verdict 5 on the two stem keys the frame program of the timed configuration (batch 4, 256 x 320)
    holds one conv on the fused tile per stem layer and no transform ops around it; the batch-1, 240 x 320 recording does not change."""
    from vi_depth_completion_amd import engine as E
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.pipeline import build_frame_program
    monkeypatch.setenv("VIDC_PRECISION", "fp32")
    monkeypatch.delenv("VIDC_WINOGRAD", raising=False)
    monkeypatch.delenv("VIDC_WINO_FUSED", raising=False)
    cpu = torch.device("cpu")

    def record(override, batch, H, W):
        if override is None:
            monkeypatch.delenv("VIDC_TUNING_OVERRIDE", raising=False)
        else:
            monkeypatch.setenv("VIDC_TUNING_OVERRIDE", override)
        monkeypatch.setattr(E, "_TUNING", None)
        cc = np.array([0.5 * 319.87654 * W / 320.0, 0.5 * 239.87603 * H / 240.0])          # (the principal point sets the warp's frame size)
        sn, dc = SurfaceNormalPrediction(fc_img=np.array([202.0, 202.0]), cc_img=cc).eval(), ModifiedFPN().eval()
        return build_frame_program(sn, dc, batch, H, W, cpu, dry_run=True)

    try:
        fused = record('{"%s": [5, 0], "%s": [5, 0]}' % STEM_KEYS, 4, 256, 320)
        kf = [k for k, *_ in fused.ops]
        n = 0
        for i, (kind, _r, _w, kwargs) in enumerate(fused.ops):
            if kind == "conv" and kwargs.get("wino_fused"):
                d = fused.c_ops[i].u.conv
                if d.Cin == 64 and d.H == 128 and d.W == 160:
                    assert "@wino4f" in fused.op_names[i] and d.Cout in (64, 128) and d.groups == 4 and d.B == 4 and d.w_gs == 36 * d.Cout * d.Cin
                    assert kf[i - 1] != "wino_in" and (i + 1 == len(kf) or kf[i + 1] != "wino_out")
                    n += 1
        assert n == 2
        # batch 1, 240 x 320 (tests/test_program_recording.py pins it): other keys, the same recording
        base = record(None, 1, 240, 320)
        over = record('{"%s": [5, 0], "%s": [5, 0]}' % STEM_KEYS, 1, 240, 320)
        assert base.op_names == over.op_names
    finally:
        E._TUNING = None
