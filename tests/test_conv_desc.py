"""The descriptor builder (_lib.conv_desc / gemm_desc) against numbers written out from the rules of include/vidc.h, one small shape per
form, and the split-K workspace rule of engine.Program.finalize.  CPU only."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vi_depth_completion_amd import _lib as L  # noqa: E402

X, WP, Y, S1, B1, S2, B2, R, YS = 0x10000, 0x20000, 0x30000, 0x40000, 0x41000, 0x42000, 0x43000, 0x50000, 0x60000


def _check(d, **want):
    """Every field of `d`: the ones named as given, the others zero / NULL (splitk and dilation 1)."""
    exp = {f: 0 for f, _ in L.ConvDesc._fields_}
    exp.update(splitk=1, dilation=1)
    exp.update(want)
    assert {f: getattr(d, f) or 0 for f, _ in L.ConvDesc._fields_} == exp


def test_fp32_direct():
    # 3 groups as channel slices; Ho = (10 + 2 - 2 - 1) // 2 + 1, Wo = (12 + 2 - 2 - 1) // 2 + 1; x_gs = Cin, w_gs = Cout*KH*KW*Cin, y_gs = r_gs = p_gs = Cout
    d = L.conv_desc(2, 10, 12, 64, 32, 3, 3, 2, 1, groups=3, x=X, w=WP, y=Y, scale1=S1, shift1=B1, scale2=S2, shift2=B2, relu1=True,
                    residual=R, ldr=200, relu3=True)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, scale2=S2, shift2=B2, residual=R, B=2, H=10, W=12, Cin=64, ldx=192, Ho=5, Wo=6,
           Cout=32, ldy=96, ldr=200, KH=3, KW=3, stride=2, pad=1, flags=L.RELU1 | L.AFFINE2 | L.RESIDUAL | L.RELU3, groups=3,
           x_gs=64, w_gs=32 * 9 * 64, y_gs=32, r_gs=32, p_gs=32)
    # one affine for every group: p_gs = 0; a dilated 3x3: Ho = (10 + 2*2 - 2*2 - 1) // 1 + 1
    d = L.conv_desc(1, 10, 12, 32, 32, 3, 3, 1, 2, dilation=2, groups=2, ldx=100, ldy=80, shared_affine=True, accumulate=True)
    _check(d, B=1, H=10, W=12, Cin=32, ldx=100, Ho=10, Wo=12, Cout=32, ldy=80, KH=3, KW=3, stride=1, pad=2, flags=L.ACCUM, groups=2,
           x_gs=32, w_gs=32 * 9 * 32, y_gs=32, dilation=2)


def test_bf16x3_direct():
    # the split-bf16 image keeps every stride of the fp32 layout; the split output image goes to y_split
    d = L.conv_desc(1, 8, 8, 64, 96, 1, 1, groups=2, precision=L.PREC_BF16X3, x=X, w=WP, y=Y, scale1=S1, shift1=B1, relu1=True,
                    split_out=YS, no_f32_out=True)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, y_split=YS, B=1, H=8, W=8, Cin=64, ldx=128, Ho=8, Wo=8, Cout=96, ldy=192, KH=1, KW=1,
           stride=1, flags=L.RELU1 | L.SPLIT_OUT | L.NO_F32_OUT, groups=2, x_gs=64, w_gs=96 * 64, y_gs=96, p_gs=96, precision=L.PREC_BF16X3)


def test_bf16_direct():
    # two bf16 channels per element: Cin, ldx, x_gs halved, w_gs = Cout*KH*KW*Cin in those units; channel-sum partials in y_split
    d = L.conv_desc(2, 8, 8, 128, 64, 3, 3, 1, 1, groups=3, Ho=8, Wo=8, ldx=384, ldy=192, precision=L.PREC_BF16, x=X, w=WP, y=Y,
                    scale1=S1, shift1=B1, shared_affine=True, stats_out=YS)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, y_split=YS, B=2, H=8, W=8, Cin=64, ldx=192, Ho=8, Wo=8, Cout=64, ldy=192, KH=3, KW=3,
           stride=1, pad=1, flags=L.STATS_OUT, groups=3, x_gs=64, w_gs=64 * 9 * 64, y_gs=64, precision=L.PREC_BF16)


def test_mxfp8_direct():
    # four channels per element; a group is a data + scale plane pair: x_gs = B*H*W*Cin/128*33, w_gs = Cout*KH*KW*Cin/128*33
    d = L.conv_desc(1, 4, 6, 256, 64, 3, 3, 1, 1, groups=2, precision=L.PREC_MXFP8, x=X, w=WP, y=Y, scale1=S1, shift1=B1, relu1=True,
                    mx_out=YS, no_f32_out=True)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, y_split=YS, B=1, H=4, W=6, Cin=64, ldx=64, Ho=4, Wo=6, Cout=64, ldy=128, KH=3, KW=3,
           stride=1, pad=1, flags=L.RELU1 | L.MXFP8_OUT | L.NO_F32_OUT, groups=2, x_gs=24 * 2 * 33, w_gs=64 * 9 * 2 * 33, y_gs=64, p_gs=64,
           precision=L.PREC_MXFP8)
    with pytest.raises(AssertionError):          # an MXFP8 activation is one dense plane per group, not a channel slice
        L.conv_desc(1, 4, 6, 256, 64, 3, 3, 1, 1, groups=2, ldx=512, precision=L.PREC_MXFP8)


def test_winograd_gemm():
    # F(4x4): a 1x1 GEMM over B = H = 1, W = tiles, groups = G*36, x_gs = Cin, w_gs = Cout*Cin, y_gs = Cout, ldx = 36*G*Cin,
    # ldy = 36*G*Cout, identity epilogue shared by the groups (p_gs = 0, flags 0)
    d = L.gemm_desc(6, 128, 64, groups=2 * 36, x=X, w=WP, y=Y, scale1=S1, shift1=B1)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, B=1, H=1, W=6, Cin=128, ldx=72 * 128, Ho=1, Wo=6, Cout=64, ldy=72 * 64, KH=1, KW=1,
           stride=1, groups=72, x_gs=128, w_gs=64 * 128, y_gs=64)


def test_winograd_fused():
    # the 3x3 geometry with the fused tile; w holds 36*Cout*Cin floats of U per group
    d = L.conv_desc(1, 16, 20, 48, 32, 3, 3, 1, 1, groups=2, x=X, w=WP, y=Y, scale1=S1, shift1=B1, scale2=S2, shift2=B2, relu1=True,
                    relu2=True, wino_fused=True)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, scale2=S2, shift2=B2, B=1, H=16, W=20, Cin=48, ldx=96, Ho=16, Wo=20, Cout=32, ldy=64,
           KH=3, KW=3, stride=1, pad=1, flags=L.RELU1 | L.AFFINE2 | L.RELU2, groups=2, x_gs=48, w_gs=36 * 32 * 48, y_gs=32, p_gs=32,
           tile=L.TILE_WINO4_FUSED)


def test_weight_gradient_gemm_ungrouped():
    # dW = dY^T Xt: rows = Cout of the conv (W), K = padded pixels (Cin), N = Cin*taps of the conv (Cout); fp32 units
    d = L.gemm_desc(64, 160, 288, ldx=160, ldy=288, x=X, w=WP, y=Y, scale1=S1, shift1=B1)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, B=1, H=1, W=64, Cin=160, ldx=160, Ho=1, Wo=64, Cout=288, ldy=288, KH=1, KW=1,
           stride=1, groups=1, x_gs=160, w_gs=288 * 160, y_gs=288, p_gs=288)


def test_weight_gradient_gemm_grouped():
    # bf16 operands (two pixels per element); group g's rows of dY^T and of dW are planes of their own (X_PLANAR_GROUPS):
    # x_gs = rows * ldx, y_gs = rows * ldy, one shared affine
    d = L.gemm_desc(64, 192, 288, groups=3, ldx=192, ldy=288, precision=L.PREC_BF16, planar=True, x=X, w=WP, y=Y, scale1=S1, shift1=B1)
    _check(d, x=X, w=WP, y=Y, scale1=S1, shift1=B1, B=1, H=1, W=64, Cin=96, ldx=96, Ho=1, Wo=64, Cout=288, ldy=288, KH=1, KW=1, stride=1,
           flags=L.X_PLANAR_GROUPS, groups=3, x_gs=64 * 96, w_gs=288 * 96, y_gs=64 * 288, precision=L.PREC_BF16)


def test_streamed_tile_gets_no_workspace(monkeypatch):
    """A Winograd-product launch that the table puts on the streamed tile 40 with `splitk` = 4 group chunks needs no split-K workspace
    (vidc_conv2d_workspace_bytes = 0): finalize() must not attach one -- nor look for one, when no other conv of its stream needs one."""
    import torch
    from vi_depth_completion_amd import engine
    L.build()
    L.lib()
    # 3x3 conv 128 -> 256 channels on an 8x8 map as F(4x4): 4 tiles (<= 96 rows), Cin % 64 == 0, Cin >= 128, fp32
    monkeypatch.setenv("VIDC_TUNING_OVERRIDE", '{"M4_N256_K128_k1s1_G36": [40, 4]}')
    monkeypatch.setattr(engine, "_TUNING", None)
    net = torch.nn.Module()
    net.conv = torch.nn.Conv2d(128, 256, 3, 1, 1)
    prog = engine.Program(engine.WeightStore(net.eval()), torch.device("cpu"), 1, mode="fp32", winograd="4")
    x = prog.nhwc(8, 8, 128)
    prog.mark_output("y", prog.conv(x, "conv", relu=True, padding=1))
    prog.finalize(dry_run=True)
    (i, name), = [(i, n) for i, n in enumerate(prog.op_names) if n.startswith("conv:")]
    d = prog.c_ops[i].u.conv
    assert name.startswith("conv:conv@wino4:g96x32s:sk4:fp32 M4_N256_K128_k1s1_G36") and (d.tile, d.splitk) == (40, 4)
    assert L.lib().vidc_conv2d_workspace_bytes(ctypes.byref(d)) == 0 and not d.workspace and prog.workspaces == {}
