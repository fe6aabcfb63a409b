"""MXFP8 inference mode, host side: the format's CPU emulation on hand-computed cases, the dry-run recording of the frame program
in the mxfp8 mode against the mixed mode, the detector staying fp32, and the descriptor checks of VIDC_PREC_MXFP8 (no GPU)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_ref as R  # noqa: E402


def _block(vals, fill=0.0):
    x = torch.full((32,), fill, dtype=torch.float32)
    for i, v in vals.items():
        x[i] = v
    return x


def test_zero_block():
    codes, scales = R.quant_blocks(torch.zeros(64))
    assert codes.tolist() == [0] * 64 and scales.tolist() == [0, 0]


def test_saturation_at_448():
    # amax 511 -> E = 8 - 8 = 0: 511 saturates to 448 (0x7E), -500 to -448 (0xFE), 464 (a tie above 448) to 448; never 0x7F (NaN)
    codes, scales = R.quant_blocks(_block({0: 511.0, 1: -500.0, 2: 464.0, 3: 448.0, 4: 256.0}))
    assert scales.tolist() == [127]
    assert codes[:5].tolist() == [0x7E, 0xFE, 0x7E, 0x7E, 0x78]


def test_subnormals_round_to_nearest_even():
    # amax 1.0 -> E = -8, so x * 2^8: 2^-17 -> 2^-9 (the smallest subnormal, 0x01); 1.5 * 2^-17 -> tie -> 2 * 2^-9 (0x02);
    # 2.5 * 2^-17 -> tie -> 2 (0x02); 0.5 * 2^-17 -> tie -> 0; 7.5 * 2^-17 -> 8 * 2^-9 = 2^-6, the smallest normal (0x08)
    u = 2.0 ** -17
    codes, scales = R.quant_blocks(_block({0: 1.0, 1: u, 2: 1.5 * u, 3: 2.5 * u, 4: 0.5 * u, 5: 7.5 * u, 6: -u}))
    assert scales.tolist() == [127 - 8]
    assert codes[1:7].tolist() == [0x01, 0x02, 0x02, 0x00, 0x08, 0x81]
    assert codes[0].item() == 0x78       # 1.0 * 2^8 = 256 = 2^8 x 1.000 (exponent field 8 + 7 = 15)


def test_powers_of_two_at_block_edges():
    # each block's scale comes from its own 32 values: 2^k at both edges of block 0, 2^-k at both edges of block 1
    x = torch.zeros(64)
    x[0], x[31], x[32], x[63] = 2.0 ** 20, -(2.0 ** 19), 2.0 ** -20, 2.0 ** -21
    codes, scales = R.quant_blocks(x)
    assert scales.tolist() == [127 + 12, 127 - 28]
    assert codes[[0, 31, 32, 63]].tolist() == [0x78, 0xF0, 0x78, 0x70]       # 256, -128, 256, 128
    v = R.dequant_blocks(codes, scales)
    assert v[[0, 31, 32, 63]].tolist() == [2.0 ** 20, -(2.0 ** 19), 2.0 ** -20, 2.0 ** -21]


def test_tiny_block_uses_the_smallest_scale():
    # amax below 2^-118: E clamps to -127 (byte 0); 2^-120 * 2^127 = 128 (0x70), 2^-130 * 2^127 = 0.125 (0x20)
    codes, scales = R.quant_blocks(_block({0: 2.0 ** -120, 1: 2.0 ** -130}))
    assert scales.tolist() == [0]
    assert codes[:2].tolist() == [0x70, 0x20]
    assert R.dequant_blocks(codes, scales)[0].item() == 2.0 ** -120


def test_round_trip_error_is_bounded():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 256, generator=g) * torch.exp2(torch.randint(-20, 20, (64, 8), generator=g).float()).repeat_interleave(32, 1)
    codes, scales = R.quant_blocks(x)
    v = R.dequant_blocks(codes, scales)
    amax = x.reshape(64, 8, 32).abs().amax(-1, keepdim=True).expand(64, 8, 32).reshape(64, 256).double()
    err = (v - x.double()).abs()
    sat = (x.double().abs() - 448.0 * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)).clamp(min=0)   # amax * 2^-E is in [256, 512)
    assert (err <= torch.maximum(x.double().abs() * 2.0 ** -4, amax * 2.0 ** -17) + sat).all()
    assert (sat > 0).any() and (err[sat == 0] <= torch.maximum(x.double().abs() * 2.0 ** -4, amax * 2.0 ** -17)[sat == 0]).all()
    assert scales.max().item() < 0xFF


# ---- engine: the mxfp8 mode recorded on CPU ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vi_depth_completion_amd import _lib as L
    try:
        return L.lib()
    except Exception as e:     # the library is built by __graft_entry__.build()
        pytest.skip("libvidc.so not built: %s" % e)


def _frame_program(mode):
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.pipeline import build_frame_program
    old = os.environ.get("VIDC_PRECISION")
    os.environ["VIDC_PRECISION"] = mode
    try:
        sn = SurfaceNormalPrediction(fc_img=np.array([202.0, 202.0])).eval()
        dc = ModifiedFPN().eval()
        return build_frame_program(sn, dc, 1, 240, 320, torch.device("cpu"), dry_run=True)
    finally:
        if old is None:
            os.environ.pop("VIDC_PRECISION")
        else:
            os.environ["VIDC_PRECISION"] = old


@pytest.fixture(scope="module")
def frame_programs(lib):
    return {m: _frame_program(m) for m in ("mixed", "mxfp8")}


def _layers(prog):
    """conv layer (first key) -> (precision, Winograd m) of its GEMM; the transform ops of a Winograd layer carry its m."""
    out = {}
    for kind, _r, _w, kw in prog.ops:
        if kind == "conv":
            out[kw["keys"][0]] = (kw["precision"], kw.get("wino", 0) or (5 if kw.get("wino_fused") else 0))
    return out


def test_mxfp8_layer_selection(frame_programs):
    from vi_depth_completion_amd import _lib as L
    from vi_depth_completion_amd import engine
    mixed, mx = _layers(frame_programs["mixed"]), _layers(frame_programs["mxfp8"])
    assert set(mixed) == set(mx)
    n_mx = 0
    for kind, _r, _w, kw in frame_programs["mxfp8"].ops:
        if kind != "conv":
            continue
        co, ci, kh, kwid, Ho, Wo = kw["geom"]
        flops = 2 * Ho * Wo * co * ci * kh * kwid * len(kw["keys"])
        key = kw["keys"][0]
        if kw.get("wino") or kw.get("wino_fused"):
            assert not engine.mxfp8_layer(key, co, ci, 2 * Ho * Wo * co * ci * 9 * len(kw["keys"])) and mx[key] == mixed[key]
        elif engine.mxfp8_layer(key, co, ci, flops):
            assert kw["precision"] == L.PREC_MXFP8, key
            n_mx += 1
        else:
            assert mx[key] == mixed[key], key      # every other layer: the mixed mode's precision and Winograd choice
    # ResNet-101 layers 2-4 (all four pyramids per grouped launch); layer 1 and the decoders are excluded for accuracy
    names = [k for k, (p, _m) in mx.items() if p == L.PREC_MXFP8]
    assert n_mx == len(names) and n_mx >= 90
    for part in ("layer2.", "layer3.", "layer4."):
        assert any(part in k for k in names), part
    assert engine.MXFP8_EXCLUDED == ("layer1.", "_upsamping.", "feature_concat.")
    assert not any(e in k for k in names for e in engine.MXFP8_EXCLUDED)
    # an MXFP8 conv never carries the split-bf16 epilogue (a bf16x3 reader of its output gets a split launch)
    for kind, _r, _w, kw in frame_programs["mxfp8"].ops:
        if kind == "conv" and kw["precision"] == L.PREC_MXFP8:
            assert not kw["flags"] & L.SPLIT_OUT and kw.get("split_out") is None


def test_mxfp8_convs_read_mxfp8_images(frame_programs):
    from vi_depth_completion_amd import _lib as L
    prog = frame_programs["mxfp8"]
    images = {}
    for kind, _r, _w, kw in prog.ops:
        if kind == "quant":
            images[kw["y"].buf] = "quant"
        elif kind == "conv" and kw.get("mx_out") is not None:
            assert kw["precision"] == L.PREC_MXFP8 and kw["flags"] & L.MXFP8_OUT
            images[kw["mx_out"].buf] = "conv"
        if kind == "conv" and kw["precision"] == L.PREC_MXFP8:
            assert kw["x"].buf in images, kw["keys"][0]       # produced before this conv reads it
    assert prog.n_fused_quants > 0 and "conv" in images.values() and "quant" in images.values()
    # the descriptors: four channels per element, group planes, the planner's MXFP8 tilings
    for op, (kind, _r, _w, kw) in zip(prog.c_ops, prog.ops):
        if kind == "conv" and kw["precision"] == L.PREC_MXFP8:
            d = op.u.conv
            co, ci, kh, kwid, Ho, Wo = kw["geom"]
            assert d.precision == 3 and d.Cin == ci // 4 and d.ldx == ci // 4 and d.tile in L.MXFP8_TILES
            assert d.x_gs == d.B * d.H * d.W * ci * 33 // 128 and d.w_gs == co * kh * kwid * ci * 33 // 128
            if d.flags & L.MXFP8_OUT:
                assert d.y_split != 0


def test_levels_have_one_split_image_each(frame_programs):
    """The decoders' bf16x3 convs read channel slices of the pyramid levels: as in the mixed mode, each level gets ONE split image of all its
    groups (pipeline.build_frame_program), written by a split launch behind the MXFP8 producers of levels 2-4 and by the bf16x3 producer's
    epilogue for level 1 -- no split launch of a slice."""
    prog = frame_programs["mxfp8"]
    splits = [kw["x"] for kind, _r, _w, kw in prog.ops if kind == "split"]
    assert len(splits) == 3 and all(x.G == 4 and x.ch_off == 0 and x.ld == 4 * x.C for x in splits)


def test_mixed_mode_recording_is_unchanged(frame_programs):
    prog = frame_programs["mixed"]
    assert not any(kind == "quant" for kind, _r, _w, _kw in prog.ops)
    assert all(kw["precision"] in (0, 1) for kind, _r, _w, kw in prog.ops if kind == "conv")


def test_detector_stays_fp32_under_mxfp8(lib, monkeypatch):
    monkeypatch.setenv("VIDC_PRECISION", "mxfp8")
    from vi_depth_completion_amd.networks.plane_mask_rcnn import GeneralizedRCNN
    from vi_depth_completion_amd import engine
    assert engine.precision_mode() == "mxfp8"
    det = GeneralizedRCNN().eval()
    prog = det.build_dense(1, 240, 320, torch.device("cpu"), dry_run=True)
    convs = [kw for kind, _r, _w, kw in prog.ops if kind == "conv"]
    assert prog.mode == "fp32" and convs and all(kw["precision"] == 0 and not kw.get("wino") for kw in convs)
    assert not any(kind == "quant" for kind, _r, _w, _kw in prog.ops)


def _desc(L):
    d = L.ConvDesc()
    d.x = d.w = d.y = d.scale1 = d.shift1 = 8
    d.B, d.H, d.W, d.Ho, d.Wo, d.Cout, d.ldy = 1, 8, 8, 8, 8, 64, 64
    d.Cin, d.ldx = 32, 32            # 128 channels in units of four
    d.KH = d.KW = d.stride = d.groups = d.splitk = 1
    d.precision = L.PREC_MXFP8
    return d


def test_mxfp8_descriptor_validation(lib):
    from vi_depth_completion_amd import _lib as L
    d = _desc(L)
    d.Cin, d.ldx = 16, 16            # 64 channels: not a whole 128-channel unit
    assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"Cin" in lib.vidc_last_error()
    d = _desc(L)
    d.ldx = 48                       # 192-channel rows: the scale rows would not be dword-aligned
    assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"ldx" in lib.vidc_last_error()
    for flag in (L.STATS_OUT, L.SPLIT_OUT, L.X_PLANAR_GROUPS):
        d = _desc(L)
        d.flags, d.y_split = flag, 8
        assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"MXFP8" in lib.vidc_last_error()
    for tile in (1, 14, 33, 40, 42):  # no MXFP8 instance: 128x128, loader-wave, pipelined, streamed, Winograd
        d = _desc(L)
        d.tile = tile
        assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"MXFP8" in lib.vidc_last_error()
    d = L.ConvDesc()                 # MXFP8_OUT is an epilogue of the MXFP8 kernel only
    d.x = d.w = d.y = d.scale1 = d.shift1 = d.y_split = 8
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout, d.ldy = 1, 8, 8, 128, 128, 8, 8, 128, 128
    d.KH = d.KW = d.stride = d.groups = d.splitk = 1
    d.flags = L.MXFP8_OUT
    assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"MXFP8_OUT" in lib.vidc_last_error()
    assert lib.vidc_quant_mxfp8(8, 8, 10, 96, 96, 1, None) == -2 and b"128" in lib.vidc_last_error()
    assert lib.vidc_pack_conv_weight_mxfp8(8, 8, 64, 64, 3, 3, None) == -2 and b"128" in lib.vidc_last_error()


def test_mxfp8_plan_skips_the_128x128_tiling(lib):
    from vi_depth_completion_amd import _lib as L
    d = L.ConvDesc()
    d.B, d.Ho, d.Wo, d.Cout, d.Cin, d.KH, d.KW, d.groups = 1, 1, 80000, 1024, 64, 1, 1, 1
    assert lib.vidc_conv2d_plan(C.byref(d)) == 0 and d.tile == 1       # what the fp32 / bf16 modes pick for a huge GEMM
    d.precision = L.PREC_MXFP8
    assert lib.vidc_conv2d_plan(C.byref(d)) == 0 and d.tile in L.MXFP8_TILES
