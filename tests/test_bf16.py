"""Plain-bf16 inference mode on the GPU (VIDC_PRECISION=bf16, VIDC_PREC_BF16 with the VIDC_BF16_OUT epilogue): the weight packer and the
cast op bit for bit against the CPU emulation (tests/bf16_ref.py), the MFMA lane map with exact integer data on every tile, conv parity
against a float64 conv of the bf16-rounded operands, the fused VIDC_BF16_OUT image against the stand-alone cast, the torch op, partner
independence of the frame stream, the whole-path accuracy against the fp32 path and the MXFP8 mode, and the frame program run eagerly
and as a captured graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402

from vi_depth_completion_amd import _lib as L, ops  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


@pytest.mark.parametrize("shape", [(64, 128, 1, 1), (96, 256, 3, 3), (32, 192, 3, 3)])
def test_weight_packer_bit_identical_to_emulation(shape):
    g = torch.Generator().manual_seed(2)
    w = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-12, 12, shape[:2], generator=g).float())[:, :, None, None]
    got = ops.pack_conv_weight_bf16(w.to(DEV))
    assert torch.equal(R.tensor_bits(got), R.pack_weight(w))
    # ... and to pack kind 4 of the batched packer, whose bytes it promises
    co, ci, kh, kw = shape
    wd, out = w.to(DEV), torch.empty(co, kh * kw * ci, dtype=torch.bfloat16, device=DEV)
    item = (L.PackItem * 1)()
    item[0].w, item[0].packed, item[0].Cout, item[0].Cin, item[0].KH, item[0].KW, item[0].kind, item[0].block_begin = L.ptr(wd), L.ptr(out), co, ci, kh, kw, 4, 0
    dev = torch.frombuffer(bytearray(bytes(item)), dtype=torch.uint8).to(DEV)
    L.check(L.lib().vidc_pack_conv_weights_batched(L.ptr(dev), 1, L.lib().vidc_pack_item_blocks(co, ci, kh, kw, 4), L.current_stream()), "pack")
    assert torch.equal(R.tensor_bits(out), R.tensor_bits(got))


class _NoWeights:
    def raw(self, key):
        raise KeyError(key)


def test_cast_op_through_a_program():
    """Program.cast of a whole tensor and of a channel slice of it (ONE launch, the slice is a view of the image), bit for bit."""
    from vi_depth_completion_amd import engine
    g = torch.Generator().manual_seed(4)
    B, H, W, Cc = 2, 5, 7, 192
    x = torch.randn(B, H, W, Cc, generator=g) * torch.exp2(torch.randint(-20, 20, (B, H, W, Cc), generator=g).float())
    prog = engine.Program(_NoWeights(), torch.device(DEV), B, mode="bf16")
    t = prog.nhwc(H, W, Cc)
    prog.pinned.add(t.buf)
    img = prog.cast(t)
    sl = prog.cast(engine.T(t.buf, B, H, W, 64, 1, t.ld, 128))
    assert sl.buf == img.buf and (sl.ch_off, sl.ld, sl.esz) == (128, Cc, 2) and [k for k, _r, _w, _kw in prog.ops] == ["cast"]
    prog.pinned.add(img.buf)
    prog.finalize()
    prog.tensor(t).copy_(x.to(DEV))
    prog.run()
    torch.cuda.synchronize()
    got = prog.storage[img.buf][: B * H * W * Cc // 2].view(torch.bfloat16).reshape(B, H, W, Cc)
    assert torch.equal(R.tensor_bits(got), R.bits(x))
    assert torch.equal(R.tensor_bits(got[..., 128:192]), R.bits(x[..., 128:192]))
    assert torch.equal(R.tensor_bits(ops.cast_bf16(x.to(DEV))), R.bits(x))


def _affine(co, g, G=1):
    return (torch.rand(G * co, generator=g) + 0.5), (torch.rand(G * co, generator=g) - 0.5)


def _reference(x, w_list, s1, b1, stride, pad, dil, relu1=False, residual=None, relu3=False):
    """float64 conv of the bf16-ROUNDED operands (per group), the epilogue, and the per-output bound 1e-5 * |s1| * sum |x^ w^| (products
    of two bf16 values are exact in fp32; the error is the fp32 accumulation's)."""
    B, H, W, ld = x.shape
    G = len(w_list)
    Cc = ld // G
    xq = R.rounded(x).double().permute(0, 3, 1, 2)
    outs, bounds = [], []
    for gi, w in enumerate(w_list):
        wq = R.rounded(w).double()
        xi = xq[:, gi * Cc:(gi + 1) * Cc]
        outs.append(F.conv2d(xi, wq, stride=stride, padding=pad, dilation=dil))
        bounds.append(F.conv2d(xi.abs(), wq.abs(), stride=stride, padding=pad, dilation=dil))
    acc, bnd = torch.cat(outs, 1).permute(0, 2, 3, 1), torch.cat(bounds, 1).permute(0, 2, 3, 1)
    y = acc * s1.double() + b1.double()
    if relu1:
        y = y.clamp(min=0)
    if residual is not None:
        y = y + residual.double()
        if relu3:
            y = y.clamp(min=0)
    return y, 1e-5 * bnd * s1.double().abs() + 1e-30


def _run(x, w_list, s1, b1, k, stride, pad, dil, tile=0, splitk=1, **kw):
    wp = torch.cat([ops.pack_conv_weight_bf16(w.to(DEV)).reshape(-1) for w in w_list])
    return ops.conv2d_bn_act(x.to(DEV), wp, s1.to(DEV), b1.to(DEV), k, k, stride=stride, pad=pad, dilation=dil, groups=len(w_list),
                             precision=L.PREC_BF16, tile=tile, splitk=splitk, **kw)


def test_mfma_lane_map_exact_integers():
    """Small integers (exact in bf16) and an asymmetric B: every product and partial sum is exact in fp32, so the conv must reproduce
    the float64 result bit for bit on every tile.  A wrong operand lane map, k order inside a fragment or channel half of the 64-channel
    unit moves values and fails this."""
    g = torch.Generator().manual_seed(3)
    B, H, W, ci, co = 1, 4, 8, 128, 64                         # M = 32 rows, two 64-channel K units
    x = torch.randint(-7, 8, (B, H, W, ci), generator=g).float()
    w = torch.randint(-6, 7, (co, ci, 1, 1), generator=g).float()
    w[:, ::32] = (torch.arange(co)[:, None] % 7 + 8).float()[..., None, None].expand(co, ci // 32, 1, 1)
    s1, b1 = torch.ones(co), torch.zeros(co)
    assert torch.equal(R.rounded(x), x) and torch.equal(R.rounded(w), w)     # the operands are exact
    ref = torch.einsum("bhwc,oc->bhwo", x.double(), w[:, :, 0, 0].double())
    for tile in L.BF16_TILES:
        y = _run(x, [w], s1, b1, 1, 1, 0, 1, tile=tile).cpu().double()
        assert torch.equal(y, ref), "tile %s: %d outputs differ" % (L.TILE_NAMES[tile], int((y != ref).sum()))


CASES = [  # B, H, W, ci, co, k, stride, pad, dil, G
    (1, 12, 20, 128, 64, 1, 1, 0, 1, 1),
    (1, 16, 16, 256, 64, 1, 2, 0, 1, 1),
    (1, 10, 14, 64, 64, 3, 1, 1, 1, 1),        # one 64-channel K unit per tap
    (2, 15, 20, 128, 96, 3, 2, 1, 1, 1),
    (1, 12, 16, 128, 64, 3, 1, 2, 2, 1),       # dilated 3x3 (the ASPP branches of the DORN normal net)
    (1, 10, 12, 64, 64, 3, 1, 1, 1, 3),        # three groups
    (4, 15, 20, 256, 128, 1, 1, 0, 1, 4),      # four groups, batch 4 (the frame program's 1x1s)
]


@pytest.mark.parametrize("case", CASES)
def test_conv_parity(case):
    B, H, W, ci, co, k, st, pad, dil, G = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, W, G * ci, generator=g)
    ws = [torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5 for _ in range(G)]
    s1, b1 = _affine(co, g, G)
    ref, tol = _reference(x, ws, s1, b1, st, pad, dil, relu1=True)
    y = _run(x, ws, s1, b1, k, st, pad, dil, relu1=True).cpu().double()
    worst = float(((y - ref).abs() / tol).max())
    print("bf16 conv parity %s: worst error / bound %.3f" % (case, worst))
    assert y.shape == ref.shape and ((y - ref).abs() <= tol).all(), worst


@pytest.mark.parametrize("tile,splitk", [(7, 4), (6, 2), (4, 3)])
def test_conv_parity_split_k(tile, splitk):
    g = torch.Generator().manual_seed(10 + tile)
    x = torch.randn(1, 6, 8, 512, generator=g)
    w = torch.randn(64, 512, 3, 3, generator=g) * 0.02
    s1, b1 = _affine(64, g)
    ref, tol = _reference(x, [w], s1, b1, 1, 1, 1)
    ws = torch.zeros(1 << 20, device=DEV)
    y = _run(x, [w], s1, b1, 3, 1, 1, 1, tile=tile, splitk=splitk, workspace=ws).cpu().double()
    worst = float(((y - ref).abs() / tol).max())
    print("bf16 split-K parity tile %d x %d: worst error / bound %.3f" % (tile, splitk, worst))
    assert ((y - ref).abs() <= tol).all(), worst


BF16_OUT_FLAGS = ["relu1", "residual_relu3", "affine2_relu2", "accum"]


@pytest.fixture(scope="module")
def out_case():
    g = torch.Generator().manual_seed(5)
    B, H, W, ci, co, G = 2, 9, 11, 128, 64, 2                  # M = 198 rows: no multiple of any tile height
    return {"x": torch.randn(B, H, W, G * ci, generator=g), "ws": [torch.randn(co, ci, 3, 3, generator=g) * 0.04 for _ in range(G)],
            "aff": _affine(co, g, G), "aff2": _affine(co, g, G), "res": torch.randn(B, H, W, G * co, generator=g),
            "y0": torch.randn(B, H, W, G * co, generator=g), "shape": (B, H, W, G * co)}


def _flag_kwargs(c, flags):
    kw = {}
    if flags == "relu1":
        kw = dict(relu1=True)
    elif flags == "residual_relu3":
        kw = dict(residual=c["res"].to(DEV), relu3=True)
    elif flags == "affine2_relu2":
        kw = dict(relu1=True, scale2=c["aff2"][0].to(DEV), shift2=c["aff2"][1].to(DEV), relu2=True)
    elif flags == "accum":
        kw = dict(accumulate_into=c["y0"].to(DEV).clone())
    return kw


@pytest.mark.parametrize("tile,splitk", [(0, 1), (4, 3), (5, 1)], ids=["planned", "splitk3", "K2tile"])
@pytest.mark.parametrize("flags", BF16_OUT_FLAGS)
def test_bf16_out_image(out_case, flags, tile, splitk):
    """VIDC_BF16_OUT: the image is the bits ops.cast_bf16 makes of the SAME launch's fp32 output (groups at channel g * Cout of dense
    rows), the fp32 output is what the launch without the flag writes, and with VIDC_NO_F32_OUT the image is the same bits while y is
    left alone -- under the planned tile, under split-K (the tile that takes the last ticket writes the image) and under a _K2 tile."""
    c = out_case
    s1, b1 = c["aff"]
    plain = _run(c["x"], c["ws"], s1, b1, 3, 1, 1, 1, tile=tile, splitk=splitk, **_flag_kwargs(c, flags))
    img = torch.zeros(c["shape"], dtype=torch.bfloat16, device=DEV)
    y = _run(c["x"], c["ws"], s1, b1, 3, 1, 1, 1, tile=tile, splitk=splitk, bf16_out=img, **_flag_kwargs(c, flags))
    assert torch.equal(y, plain)
    assert torch.equal(R.tensor_bits(img), R.tensor_bits(ops.cast_bf16(y))) and torch.equal(R.tensor_bits(img), R.bits(y.cpu()))
    if flags in ("relu1", "residual_relu3"):                    # ... and y is the conv it should be
        ref, tol = _reference(c["x"], c["ws"], s1, b1, 1, 1, 1, relu1=flags == "relu1", residual=c["res"] if flags != "relu1" else None, relu3=True)
        assert ((y.cpu().double() - ref).abs() <= tol).all(), float(((y.cpu().double() - ref).abs() / tol).max())
    img2 = torch.zeros_like(img)
    kw = _flag_kwargs(c, flags)
    keep = kw["accumulate_into"].clone() if flags == "accum" else None
    y2 = _run(c["x"], c["ws"], s1, b1, 3, 1, 1, 1, tile=tile, splitk=splitk, bf16_out=img2, no_f32_out=True, **kw)
    assert torch.equal(R.tensor_bits(img2), R.tensor_bits(img))
    if keep is not None:
        assert torch.equal(y2, keep)                            # the fp32 store was skipped: the accumulator still holds its input


def test_bf16_out_refused_combinations(out_case):
    c = out_case
    B, H, W, ld = c["x"].shape
    x, img = ops.cast_bf16(c["x"].to(DEV)), torch.zeros(c["shape"], dtype=torch.bfloat16, device=DEV)
    wp = torch.cat([ops.pack_conv_weight_bf16(w.to(DEV)).reshape(-1) for w in c["ws"]])
    y = torch.zeros(c["shape"], device=DEV)
    s1, b1 = (t.to(DEV) for t in c["aff"])
    d = L.conv_desc(B, H, W, ld // 2, 64, 3, 3, 1, 1, groups=2, precision=L.PREC_BF16, x=L.ptr(x), w=L.ptr(wp), y=L.ptr(y), scale1=L.ptr(s1),
                    shift1=L.ptr(b1), bf16_out=L.ptr(img))
    L.plan(d)
    d.splitk = 1
    for extra in (L.SPLIT_OUT, L.MXFP8_OUT, L.STATS_OUT):
        d.flags = L.BF16_OUT | extra
        assert L.lib().vidc_conv2d_bn_act(C.byref(d), L.current_stream()) == -2, extra
    d.flags = L.BF16_OUT
    L.check(L.lib().vidc_conv2d_bn_act(C.byref(d), L.current_stream()), "conv")
    torch.cuda.synchronize()
    assert torch.equal(R.tensor_bits(img), R.bits(y.cpu())) and float(y.abs().max()) > 0


def test_torch_op_precision_2():
    import vi_depth_completion_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 10, 12, 128, generator=g)
    w = torch.randn(64, 128, 3, 3, generator=g) * 0.04
    s1, b1 = _affine(64, g)
    y = torch.ops.vidc.conv2d_bn_act(x.to(DEV), w.to(DEV), s1.to(DEV), b1.to(DEV), 1, 1, True, 2)
    ref, tol = _reference(x, [w], s1, b1, 1, 1, 1, relu1=True)
    assert y.dtype == torch.float32 and ((y.cpu().double() - ref).abs() <= tol).all()
    with pytest.raises(RuntimeError, match="Winograd"):
        torch.ops.vidc.conv3x3_winograd(x.to(DEV), w.to(DEV), s1.to(DEV), b1.to(DEV), 4, True, 2)


# ---- the pipelines in the bf16 mode --------------------------------------------------------------------------------------------
def _pipe(seeded_weights):
    from vi_depth_completion_amd.pipeline import DepthCompletionPipeline, FixedPlaneMask
    p = DepthCompletionPipeline(enriched_samples=200)
    p.load_state_dicts(seeded_weights["sn"], seeded_weights["dc"])
    p.plane_masks_extraction = FixedPlaneMask(S.plane_id_map(240, 320))
    return p


def _frames(frame0, n):
    return [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in S.synthetic_batch(1, 240, 320, 1234, frame0=frame0 + i).items()} for i in range(n)]


def test_partner_independence_in_bf16(seeded_weights, monkeypatch):
    """A frame's depth does not depend on its partners, its slot, the number of lanes or the run: rounding is per value, and the first /
    drain ticks (group variants of the 4-group launches, their bf16 images offset by two bytes per channel) compute the same bits."""
    monkeypatch.setenv("VIDC_PRECISION", "bf16")
    pipe = _pipe(seeded_weights)
    frames = _frames(500, 5)
    rng_of = lambda f: np.random.RandomState(7000 + f)      # noqa: E731

    def run(first, last, lanes, Fl):
        return [o.cpu() for o in pipe.run_interleaved(iter(frames[first:last]), lanes=lanes, frames_per_launch=Fl, frame_rng=lambda i: rng_of(first + i))]

    for Fl in (1, 4):
        ref = run(0, 5, 1, Fl)
        assert all(bool(torch.isfinite(o).all()) for o in ref) and not torch.equal(ref[0], ref[1])
        assert torch.equal(run(0, 5, 3, Fl)[2], ref[2]) and torch.equal(run(0, 5, 1, Fl)[0], ref[0])       # lanes; a second run
        got = run(1, 5, 1, Fl)                                                                             # other partners and slots
        assert all(torch.equal(ref[f], got[f - 1]) for f in range(1, 5))


def test_whole_path_accuracy_against_fp32_and_mxfp8(seeded_weights, golden_dir, monkeypatch):
    """The demo frames with seeded weights through _call_cnn in fp32, mxfp8 and bf16.  Bars: every bf16 frame within 5 % relative depth
    RMSE of the fp32 output (the project's bar for an opt-in reduced-precision mode), and the worst bf16 frame no worse than the worst
    mxfp8 frame of the same run.  The figures (and the mean angle between the normals) are printed for the record: DESIGN 4.6b."""
    from test_frames_per_launch import _golden_batch, _golden_names
    names = _golden_names(golden_dir)
    fs = [np.load(os.path.join(golden_dir, n + ".npz")) for n in names]
    out = {}
    for mode in ("fp32", "mxfp8", "bf16"):
        monkeypatch.setenv("VIDC_PRECISION", mode)
        pipe = _pipe(seeded_weights)
        res = []
        for f, n in zip(fs, names):
            pipe.rng = np.random.RandomState(int(f["np_seed"]))
            taps = {}
            d = pipe._call_cnn(_golden_batch(f, n), taps=taps).cpu().double()
            res.append((d, taps["normals"].cpu().double()))
        out[mode] = res
    worst = {}
    for mode in ("mxfp8", "bf16"):
        rel, ang = [], []
        for (d32, n32), (d8, n8) in zip(out["fp32"], out[mode]):
            rel.append(float((d8 - d32).pow(2).mean().sqrt() / d32.pow(2).mean().sqrt()))
            cos = (F.normalize(n32, dim=1) * F.normalize(n8, dim=1)).sum(1).clamp(-1, 1)
            ang.append(float(torch.rad2deg(torch.acos(cos)).mean()))
        print("%s vs fp32 over %d frames: relative depth RMSE mean %.5f max %.5f (per frame %s); mean normal angle %.3f deg (max frame %.3f)"
              % (mode, len(rel), np.mean(rel), np.max(rel), " ".join("%.5f" % r for r in rel), np.mean(ang), np.max(ang)))
        worst[mode] = rel
    assert len(worst["bf16"]) >= 8 and max(worst["bf16"]) <= 0.05
    assert max(worst["bf16"]) <= max(worst["mxfp8"])


def test_frame_program_eager_and_captured(seeded_weights, monkeypatch):
    """The tick program recorded in the bf16 mode (dry_run=False): an eager run and a replay of its captured graph give the same bits."""
    monkeypatch.setenv("VIDC_PRECISION", "bf16")
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.pipeline import build_frame_program
    dev = torch.device(DEV)
    sn = SurfaceNormalPrediction(fc_img=np.array([202.0, 202.0]), cc_img=np.array([0.5 * 319.87654, 0.5 * 239.87603])).to(dev).eval()
    dc = ModifiedFPN().to(dev).eval()
    for m, sd in ((sn, seeded_weights["sn"]), (dc, seeded_weights["dc"])):
        state = m.state_dict()
        state.update(sd)
        m.load_state_dict(state)
    prog = build_frame_program(sn, dc, 1, 240, 320, dev)
    assert prog.mode == "bf16" and prog.n_fused_casts >= 100 and sum(1 for k, _r, _w, _kw in prog.ops if k == "cast") == 8
    b = S.synthetic_batch(1, 240, 320, 1234)
    g = torch.Generator().manual_seed(8)
    ins = {"sn_image": b["image"], "dc_image": b["image"], "gravity": b["gravity"].reshape(-1), "aligned": b["aligned_direction"].reshape(-1),
           "dc_normal": F.normalize(torch.randn(1, 3, 240, 320, generator=g), dim=1), "dc_depth": b["sparse_depth"]}

    def fill():
        for name, v in ins.items():
            t = prog.inputs[name]
            prog.storage[t.buf][: v.numel()].copy_(v.reshape(-1).float().to(dev))

    side = torch.cuda.Stream()
    res = []
    with torch.cuda.stream(side):
        for how in ("eager", "graph"):
            fill()
            if how == "eager":
                prog.run()
            else:
                prog.capture()
                fill()                                          # (capturing runs nothing; dc_normal is rewritten by every run)
                prog.launch()
            side.synchronize()
            res.append({k: prog.tensor(t).clone() for k, t in prog.outputs.items()})
    for k in res[0]:
        assert bool(torch.isfinite(res[0][k]).all()) and float(res[0][k].abs().max()) > 0 and torch.equal(res[0][k], res[1][k]), k
