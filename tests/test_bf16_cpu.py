"""Plain-bf16 inference mode (VIDC_PRECISION=bf16), host side: the rounding emulation on hand-computed cases, the dry-run recording of
the frame program and of the stand-alone networks in the bf16 mode (layer selection, the cast -> VIDC_BF16_OUT fold, the safety of
VIDC_NO_F32_OUT, the descriptors), the other modes' recordings left alone, and the descriptor checks of VIDC_BF16_OUT (no GPU)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402


def test_rounding_emulation_on_hand_computed_cases():
    # 1 + 2^-8 is a tie between 1.0 (mantissa even) and 1 + 2^-7: down; 1 + 3 * 2^-8 is a tie between odd and even: up to 1 + 2^-6
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 0.0, -0.0, 3.0e38, 2.0 ** -130])
    assert R.bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xBF80, 0x0000, 0x8000, 0x7F62, 0x0008]          # (2^-130 is the fp32 subnormal 2^19 * 2^-149)
    assert R.rounded(x)[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    g = torch.Generator().manual_seed(0)
    y = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-30, 30, (4096,), generator=g).float())
    assert torch.equal(R.bits(y), R.tensor_bits(y.to(torch.bfloat16)))          # torch's own cast rounds the same way
    w = torch.arange(2 * 128 * 9, dtype=torch.float32).reshape(2, 128, 3, 3)
    p = R.packed_weight_order(w)
    # row o, unit cu, tap (kh, kw), lane c: w[o][64 cu + c][kh][kw]
    assert p.shape == (2, 1152) and p[1, (1 * 9 + 5) * 64 + 7].item() == w[1, 64 + 7, 1, 2].item()


# ---- engine: the modes recorded on CPU -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vi_depth_completion_amd import _lib as L
    try:
        return L.lib()
    except Exception as e:     # the library is built by __graft_entry__.build()
        pytest.skip("libvidc.so not built: %s" % e)


def _record(mode):
    """{name: Program} of the frame program, the two stand-alone networks and the DORN normal network, recorded under VIDC_PRECISION=mode."""
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.networks.surface_normal_dorn import SurfaceNormalDORN
    from vi_depth_completion_amd.pipeline import build_frame_program
    old = os.environ.get("VIDC_PRECISION")
    os.environ["VIDC_PRECISION"] = mode
    try:
        sn = SurfaceNormalPrediction(fc_img=np.array([202.0, 202.0])).eval()
        dc = ModifiedFPN().eval()
        cpu = torch.device("cpu")
        out = {"frame": build_frame_program(sn, dc, 1, 240, 320, cpu, dry_run=True), "sn": sn.build_program(1, cpu, dry_run=True),
               "dc": dc.build_program(1, 240, 320, cpu, dry_run=True)}
        if mode in ("bf16", "mixed"):
            out["dorn"] = SurfaceNormalDORN(pretrained=False).eval().build_program(1, 240, 320, cpu, dry_run=True)
        return out
    finally:
        if old is None:
            os.environ.pop("VIDC_PRECISION")
        else:
            os.environ["VIDC_PRECISION"] = old


@pytest.fixture(scope="module")
def programs(lib):
    return {m: _record(m) for m in ("fp32", "mixed", "mxfp8", "bf16")}


def _layers(prog):
    """conv layer (first key) -> (precision, Winograd m) of its GEMM."""
    return {kw["keys"][0]: (kw["precision"], kw.get("wino", 0) or (5 if kw.get("wino_fused") else 0)) for kind, _r, _w, kw in prog.ops if kind == "conv"}


def test_unknown_mode_is_refused():
    from vi_depth_completion_amd import engine
    assert engine.Program(None, torch.device("cpu"), 1, mode="bf16").mode == "bf16"
    with pytest.raises(ValueError):
        engine.Program(None, torch.device("cpu"), 1, mode="bfloat16")


def test_the_mode_is_recorded(programs):
    """Every conv bf16_layer() selects is a direct VIDC_PREC_BF16 launch (at least 100 of them in the frame program: the parent recorded
    none, the mode silently fell back to fp32); every other layer makes exactly the mixed mode's choice."""
    from vi_depth_completion_amd import _lib as L
    from vi_depth_completion_amd import engine
    assert engine.BF16_EXCLUDED == ()
    for name, prog in programs["bf16"].items():
        assert prog.mode == "bf16"
        mixed, bf = _layers(programs["mixed"][name]), _layers(prog)
        assert set(mixed) == set(bf), name
        n_bf = 0
        for kind, _r, _w, kw in prog.ops:
            if kind != "conv":
                continue
            co, ci, kh, kwid, Ho, Wo = kw["geom"]
            key = kw["keys"][0]
            if kw.get("wino") or kw.get("wino_fused"):      # (geom of a Winograd GEMM is the transform domain's; the layer itself was not selected)
                assert bf[key] == mixed[key], key
            elif engine.bf16_layer(key, co, ci, 2 * Ho * Wo * co * ci * kh * kwid * len(kw["keys"])):
                assert kw["precision"] == L.PREC_BF16 and kw["x"].esz == 2, key
                n_bf += 1
            else:
                assert kw["precision"] != L.PREC_BF16 and bf[key] == mixed[key], key
        print("%s: %d of %d conv launches in bf16" % (name, n_bf, sum(1 for k, _r, _w, _kw in prog.ops if k == "conv")))
        assert n_bf >= (100 if name != "dorn" else 30), (name, n_bf)
        # a selected 3x3 layer is never a Winograd triple in this mode
        assert not any(kind in ("wino_in", "wino_out") for kind, _r, _w, _kw in prog.ops), name
    names = [k for k, (p, _m) in _layers(programs["bf16"]["frame"]).items() if p == L.PREC_BF16]
    for part in ("layer1.", "layer2.", "layer3.", "layer4.", "_upsamping.", "feature_concat.0"):
        assert any(part in k for k in names), part
    # DORN: the dilated ASPP convs and the Linear-as-1x1 qualify like any other layer
    dorn = {kw["keys"][0]: kw for kind, _r, _w, kw in programs["bf16"]["dorn"].ops if kind == "conv"}
    assert any(kw["dilation"] > 1 and kw["precision"] == L.PREC_BF16 for kw in dorn.values())
    assert any("@hwc" in k and kw["precision"] == L.PREC_BF16 for k, kw in dorn.items())


def _last_writer(prog, i, buf):
    return next((t for t in range(i - 1, -1, -1) if buf in prog.ops[t][2]), None)


def test_casts_are_folded(programs):
    """No cast launch survives behind a bf16 conv that writes the whole tensor; the survivors follow a non-conv producer (stem, max-pool,
    upsample, a program input) or a conv that fills only a slice of a concat buffer."""
    from vi_depth_completion_amd import _lib as L
    for name, prog in programs["bf16"].items():
        images = set()
        n_cast = 0
        for i, (kind, _r, _w, kw) in enumerate(prog.ops):
            if kind == "cast":
                n_cast += 1
                xs = kw["x"]
                j = _last_writer(prog, i, xs.buf)
                if j is not None and prog.ops[j][0] == "conv":
                    y = prog.ops[j][3]["y"]
                    whole = y.ch_off == 0 and y.ld == y.C * y.G and (xs.ch_off, xs.C * xs.G, xs.ld) == (0, y.C * y.G, y.ld)
                    assert not (whole and prog.ops[j][3]["precision"] == L.PREC_BF16), (name, prog.op_names[i], prog.op_names[j])
                images.add(kw["y"].buf)
            elif kind == "conv":
                if kw["precision"] == L.PREC_BF16:
                    assert kw["x"].buf in images, (name, kw["keys"][0])        # its operand image exists before it runs
                else:
                    assert kw["x"].buf not in images
                if kw.get("bf16_out") is not None:
                    assert kw["precision"] == L.PREC_BF16 and kw["flags"] & L.BF16_OUT and not kw["flags"] & (L.SPLIT_OUT | L.MXFP8_OUT | L.STATS_OUT)
                    images.add(kw["bf16_out"].buf)
                else:
                    assert not kw["flags"] & L.BF16_OUT
        print("%s: %d cast launches left, %d folded" % (name, n_cast, prog.n_fused_casts))
        assert prog.n_fused_casts >= (90 if name != "dorn" else 25) and n_cast <= 12, (name, n_cast, prog.n_fused_casts)
    # the frame program: stem output, max-pool output and the six decoder concat buffers (a conv slice + an upsample slice each)
    fp = programs["bf16"]["frame"]
    assert sum(1 for kind, _r, _w, _kw in fp.ops if kind == "cast") == 8
    # one image per pyramid level, read by both decoders as channel slices (offsets: multiples of 64 channels)
    first_sn = next(kw for k, _, _, kw in fp.ops if k == "conv" and kw["keys"][0] == "sn/feature1_upsamping.0")
    first_dc = next(kw for k, _, _, kw in fp.ops if k == "conv" and kw["keys"][0] == "dc/feature1_upsamping.0")
    assert first_sn["x"].buf == first_dc["x"].buf and (first_sn["x"].ch_off, first_dc["x"].ch_off) == (0, 256) and first_sn["x"].ld == 1024


def test_no_f32_out_is_safe(programs):
    """A conv that skips its fp32 store has no reader of the fp32 tensor: no later op reads the buffer, and it is no program output."""
    from vi_depth_completion_amd import _lib as L
    for name, prog in programs["bf16"].items():
        n = 0
        outs = {t.buf for t in prog.outputs.values()} | set(prog.pinned)
        for j, (kind, _r, _w, kw) in enumerate(prog.ops):
            if kind == "conv" and kw["flags"] & L.NO_F32_OUT:
                assert kw["flags"] & L.BF16_OUT, (name, kw["keys"][0])
                yb = kw["y"].buf
                assert yb not in outs
                assert not any(yb in prog.ops[t][1] for t in range(j + 1, len(prog.ops))), (name, kw["keys"][0])
                n += 1
            if kind == "conv" and kw["flags"] & L.RESIDUAL:      # the residual is an fp32 tensor somebody stored
                w = _last_writer(prog, j, kw["residual"].buf)
                assert w is not None and not prog.ops[w][3].get("flags", 0) & L.NO_F32_OUT, (name, kw["keys"][0])
        assert n >= (60 if name != "dorn" else 15), (name, n)


def test_bf16_descriptors(programs):
    from vi_depth_completion_amd import _lib as L
    prog = programs["bf16"]["frame"]
    for op, (kind, _r, _w, kw) in zip(prog.c_ops, prog.ops):
        if kind == "conv" and kw["precision"] == L.PREC_BF16:
            d = op.u.conv
            co, ci, kh, kwid, Ho, Wo = kw["geom"]
            x = kw["x"]
            assert d.precision == 2 and d.Cin == ci // 2 and d.ldx == x.ld // 2 and d.x_gs == ci // 2 and d.w_gs == co * kh * kwid * ci // 2
            assert d.tile in L.BF16_TILES and d.splitk >= 1
            assert d.x == prog.storage[x.buf].data_ptr() + 2 * x.ch_off
            if d.flags & L.BF16_OUT:
                assert d.y_split == prog.storage[kw["bf16_out"].buf].data_ptr() and d.ldy == len(kw["keys"]) * co
        elif kind == "cast":
            _x, _y, rows, c, ldx = L.op_args(op)
            assert op.kind == L.OP_CAST == 20 and (rows, c, ldx) == (kw["x"].B * kw["x"].H * kw["x"].W, kw["x"].C * kw["x"].G, kw["x"].ld)
            assert prog.buf_elems[kw["y"].buf] * 2 == rows * c


def test_other_modes_are_untouched(programs):
    """The fp32, mixed and mxfp8 recordings never meet the new code: no cast op, no VIDC_BF16_OUT, no VIDC_PREC_BF16, no 2-byte tensor;
    and the counts of the parent's recordings (tests/test_abi.py, tests/test_mxfp8_cpu.py) stand."""
    from vi_depth_completion_amd import _lib as L
    for mode in ("fp32", "mixed", "mxfp8"):
        for name, prog in programs[mode].items():
            assert prog.mode == mode and prog.n_fused_casts == 0
            for op, (kind, _r, _w, kw) in zip(prog.c_ops, prog.ops):
                assert kind != "cast" and op.kind != L.OP_CAST
                assert all(t.esz == 4 for t in kw.values() if hasattr(t, "esz"))
                if kind == "conv":
                    assert kw["precision"] in ((0,) if mode == "fp32" else (0, 1) if mode == "mixed" else (0, 1, 3)), (mode, name)
                    assert not kw["flags"] & L.BF16_OUT and kw.get("bf16_out") is None and not op.u.conv.flags & L.BF16_OUT
    assert not any(kind in ("split", "quant") for kind, _r, _w, _kw in programs["fp32"]["frame"].ops)
    assert not any(kind == "quant" for kind, _r, _w, _kw in programs["mixed"]["frame"].ops)
    assert sum(1 for kind, _r, _w, _kw in programs["mxfp8"]["frame"].ops if kind == "split") == 3 and programs["mxfp8"]["frame"].n_fused_quants > 0


def test_detector_stays_fp32_under_bf16(lib, monkeypatch):
    monkeypatch.setenv("VIDC_PRECISION", "bf16")
    from vi_depth_completion_amd.networks.plane_mask_rcnn import GeneralizedRCNN
    prog = GeneralizedRCNN().eval().build_dense(1, 240, 320, torch.device("cpu"), dry_run=True)
    convs = [kw for kind, _r, _w, kw in prog.ops if kind == "conv"]
    assert prog.mode == "fp32" and convs and all(kw["precision"] == 0 and not kw.get("wino") for kw in convs)
    assert not any(kind == "cast" for kind, _r, _w, _kw in prog.ops)


def _desc(L, flags=0):
    d = L.conv_desc(1, 8, 8, 128, 64, precision=L.PREC_BF16, x=8, w=8, y=8, scale1=8, shift1=8, bf16_out=8)
    d.flags |= flags
    return d


def test_bf16_out_descriptor_validation(lib):
    from vi_depth_completion_amd import _lib as L
    d = _desc(L)
    assert d.flags == L.BF16_OUT == 2048 and d.Cin == 64 and d.ldx == 64 and d.y_split == 8
    for flag in (L.SPLIT_OUT, L.MXFP8_OUT, L.STATS_OUT):        # one user of y_split per launch
        d = _desc(L, flag)
        assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2, flag
    d = _desc(L)
    d.y_split = None
    assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"BF16_OUT" in lib.vidc_last_error()
    for prec in (L.PREC_FP32, L.PREC_BF16X3):                   # an epilogue of the plain-bf16 kernel only
        d = _desc(L)
        d.precision = prec
        assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"BF16_OUT" in lib.vidc_last_error()
    d = L.conv_desc(1, 8, 8, 128, 64, precision=L.PREC_BF16, x=8, w=8, y=8, scale1=8, shift1=8, no_f32_out=True)
    d.flags |= L.NO_F32_OUT                                     # nothing would be written at all
    assert lib.vidc_conv2d_bn_act(C.byref(d), None) == -2 and b"NO_F32_OUT" in lib.vidc_last_error()
    assert lib.vidc_pack_conv_weight_bf16(8, 8, 64, 96, 3, 3, None) == -2 and b"64" in lib.vidc_last_error()
    assert lib.vidc_pack_conv_weight_bf16(None, 8, 64, 128, 3, 3, None) == -1
