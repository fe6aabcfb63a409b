"""ctypes binding of libvidc.so (the C ABI declared in include/vidc.h).

There is no fallback: if the library is missing or a call fails, a RuntimeError is raised.
`build()` compiles it in-tree with hipcc for gfx950 (also used by __graft_entry__.build()).
"""
import ctypes as C
import operator
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("VIDC_LIB_NAME", "libvidc.so"))      # (VIDC_LIB_NAME: A/B builds of tools/, never set in production)
CSRC = os.path.join(_HERE, "csrc")

WARP_PARAMS = 32
MAX_HYP = 300
PLANE_RECORD = 16
MAX_STREAMS = 4
MAX_SEGMENTS = 4
CLOCK_STAMP_WGS = 8      # VIDC_CLOCK_STAMP_WGS

# vidc_conv_flags / vidc_up_flags / vidc_op_kind / vidc_conv_tile
RELU1, AFFINE2, RELU2, RESIDUAL, RELU3, ACCUM, SPLIT_OUT, NO_F32_OUT, STATS_OUT, X_PLANAR_GROUPS, MXFP8_OUT, BF16_OUT = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048
UP_RELU, UP_ACCUM, UP_NO_F32_OUT = 1, 2, 4
OP_CONV, OP_STEM, OP_MAXPOOL, OP_UPSAMPLE, OP_HEAD, OP_WARP_PARAMS, OP_WARP_FWD, OP_WARP_INV, OP_COPY, OP_SPLIT, OP_AVGPOOL, OP_NORMALIZE, OP_DET_IM2COL, OP_NEAREST2X, _OP_RETIRED_15, OP_MASK, OP_WINO_IN, OP_WINO_OUT, OP_QUANT, OP_CAST, OP_STEM_WARPED = range(1, 22)
TILE_AUTO = 0
PREC_FP32, PREC_BF16X3, PREC_BF16, PREC_MXFP8 = 0, 1, 2, 3
TILE_KIND_AUTO, TILE_KIND_MFMA, TILE_KIND_STREAM, TILE_KIND_WINOGRAD = range(4)      # vidc_conv_tile_kind
SPLITK_COUNTERS = 16384            # VIDC_SPLITK_COUNTERS: ticket counters at the head of a split-K workspace
NONZERO_CHUNK = 1024              # VIDC_NONZERO_CHUNK
U8_UNIT, U8_NORMAL_GT, U8_NORMAL_PRED, U8_NORMAL_PRED_NYU = range(4)      # modes of vidc_u8_decode_chw
PNG_DEPTH16_F32, PNG_NORMAL8_F32, PNG_RGB8_F32, PNG_GRAY8_U8 = range(4)      # vidc_png_format
PNG_FILTER_NONE, PNG_FILTER_SUB, PNG_FILTER_UP, PNG_FILTER_AVERAGE, PNG_FILTER_PAETH, PNG_FILTER_ADAPTIVE = range(6)      # vidc_png_filter

_f32p = C.POINTER(C.c_float)


class PackItem(C.Structure):
    """vidc_pack_item (include/vidc.h)."""
    _fields_ = [("w", C.c_void_p), ("packed", C.c_void_p), ("Cout", C.c_int32), ("Cin", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
                ("kind", C.c_int32), ("reserved", C.c_int32), ("block_begin", C.c_int64)]


class TileInfo(C.Structure):
    """vidc_tile_info (include/vidc.h): one row of csrc/conv_tiles.def."""
    _fields_ = [("_name", C.c_char_p)] + [(f, C.c_int32) for f in ("bm", "bn", "wmw", "wnw", "wkw", "ns", "spec", "kind", "precisions", "planner")]
    name = property(lambda self: self._name.decode())


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p),
        ("scale1", C.c_void_p), ("shift1", C.c_void_p), ("scale2", C.c_void_p), ("shift2", C.c_void_p),
        ("residual", C.c_void_p), ("workspace", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("ldx", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32), ("ldy", C.c_int32), ("ldr", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("flags", C.c_int32), ("groups", C.c_int32),
        ("x_gs", C.c_int64), ("w_gs", C.c_int64), ("y_gs", C.c_int64), ("r_gs", C.c_int64), ("p_gs", C.c_int64),
        ("tile", C.c_int32), ("splitk", C.c_int32), ("precision", C.c_int32), ("dilation", C.c_int32),
        ("y_split", C.c_void_p),
    ]


# ---- descriptor builder: the conventions of vidc_conv_desc (include/vidc.h) are written here and nowhere else ---------------
def conv_desc(B, H, W, Cin, Cout, KH=1, KW=1, stride=1, pad=0, dilation=1, groups=1, Ho=None, Wo=None, ldx=None, ldy=None,
              precision=PREC_FP32, x=None, w=None, y=None, scale1=None, shift1=None, shared_affine=False, scale2=None, shift2=None,
              relu1=False, relu2=False, residual=None, ldr=None, relu3=False, accumulate=False, split_out=None, mx_out=None,
              stats_out=None, no_f32_out=False, wino_fused=False, bf16_out=None):
    """The vidc_conv_desc of a direct conv (include/vidc.h:110-139), or with wino_fused of the same 3x3 / stride 1 / pad 1 conv as the
    one-launch Winograd F(4x4, 3x3) (VIDC_TILE_WINO4_FUSED, vidc.h:169-174).  Without pointers it describes the geometry only.

    Geometry in channels, whatever the precision: Cin / Cout per group, ldx / ldy the row strides of x and y (default: groups * Cin /
    Cout; an MXFP8 x is `groups` planes of Cin channels), ldr the residual's (default ldy).  Pointers are ints or None.  The epilogue:
    scale1 / shift1 [groups][Cout], or one [Cout] pair for every group (shared_affine); scale2 / shift2 with relu2 (AFFINE2, RELU2);
    residual with relu3; accumulate; one image of the result in y_split: split_out (split bf16), mx_out (MXFP8), bf16_out (plain bf16)
    or stats_out (the channel-sum partials of VIDC_STATS_OUT).  no_f32_out skips the fp32 store behind split_out / mx_out / bf16_out.
    tile = AUTO, splitk = 1 (plan() chooses them), except the fused Winograd form's own tile."""
    assert sum(p is not None for p in (split_out, mx_out, stats_out, bf16_out)) <= 1
    dil = max(dilation, 1)
    Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1 if Ho is None else Ho
    Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1 if Wo is None else Wo
    ldx = (Cin if precision == PREC_MXFP8 else groups * Cin) if ldx is None else ldx
    ldy = groups * Cout if ldy is None else ldy
    flags = ((RELU1 if relu1 else 0) | (AFFINE2 | (RELU2 if relu2 else 0) if scale2 is not None else 0) |
             (RESIDUAL | (RELU3 if relu3 else 0) if residual is not None else 0) | (ACCUM if accumulate else 0) |
             (SPLIT_OUT if split_out is not None else 0) | (MXFP8_OUT if mx_out is not None else 0) | (STATS_OUT if stats_out is not None else 0) |
             (BF16_OUT if bf16_out is not None else 0) |
             (NO_F32_OUT if no_f32_out and (split_out is not None or mx_out is not None or bf16_out is not None) else 0))
    # group g reads x + g*x_gs, w + g*w_gs, writes y + g*y_gs (vidc.h:110-111): the groups are channel slices of x, y and the residual
    x_gs, w_gs = Cin, Cout * KH * KW * Cin
    if precision == PREC_BF16:          # vidc.h:182-184: two bf16 channels per element in Cin, ldx, x_gs (and so in w_gs)
        Cin, ldx = Cin // 2, ldx // 2
        x_gs, w_gs = Cin, Cout * KH * KW * Cin
    elif precision == PREC_MXFP8:       # vidc.h:192-194: four channels per element; a group is a data + scale plane pair (33 bytes per 32)
        assert ldx == Cin, "an MXFP8 activation is one dense plane of Cin channels per group"
        x_gs, w_gs = B * H * W * Cin // 128 * 33, Cout * KH * KW * Cin // 128 * 33
        Cin, ldx = Cin // 4, Cin // 4
    if wino_fused:                      # vidc.h:169-174: w holds U of 36 positions per group, re-ordered by vidc_winograd_weight_pack_fused
        w_gs = 36 * Cout * Cin
    return ConvDesc(x=x, w=w, y=y, scale1=scale1, shift1=shift1, scale2=scale2, shift2=shift2, residual=residual,
                    B=B, H=H, W=W, Cin=Cin, ldx=ldx, Ho=Ho, Wo=Wo, Cout=Cout, ldy=ldy, ldr=(0 if residual is None else ldr or ldy),
                    KH=KH, KW=KW, stride=stride, pad=pad, flags=flags, groups=groups,
                    x_gs=x_gs, w_gs=w_gs, y_gs=Cout, r_gs=(0 if residual is None else Cout),
                    p_gs=(0 if shared_affine and groups > 1 else Cout),      # (with one group p_gs is never read)
                    tile=(__getattr__("TILE_WINO4_FUSED") if wino_fused else TILE_AUTO), splitk=1, precision=precision, dilation=dil,
                    y_split=next((p for p in (split_out, mx_out, stats_out, bf16_out) if p is not None), None))


def gemm_desc(rows, K, N, groups=1, ldx=None, ldy=None, precision=PREC_FP32, planar=False, x=None, w=None, y=None, scale1=None,
              shift1=None, shared_affine=True):
    """y[g] = x[g] w[g]^T as the 1x1 conv of vidc_conv2d_bn_act over B = H = 1, W = rows (the "rows as W" GEMM): K and N in channels
    per group, epilogue scale1 / shift1 only.  The Winograd products (vidc.h:223-224: rows = tiles, groups = G * (m+2)^2, an identity
    affine shared by the groups) and the weight-gradient GEMMs of the training step (rows of dY^T times rows of the transposed im2col).
    planar: group g's rows of x and of y are planes of their own (X_PLANAR_GROUPS, vidc.h:96-97) instead of channel slices."""
    d = conv_desc(1, 1, rows, K, N, groups=groups, ldx=ldx, ldy=ldy, precision=precision, x=x, w=w, y=y, scale1=scale1, shift1=shift1,
                  shared_affine=shared_affine)
    if planar:
        d.flags |= X_PLANAR_GROUPS
        d.x_gs, d.y_gs = rows * d.ldx, rows * d.ldy
    return d


def plan(d, tiling=None):
    """d.tile, d.splitk = `tiling` (a measured (tile, splitk)), or without one the planner's choice (vidc_conv2d_plan)."""
    if tiling is not None:
        d.tile, d.splitk = tiling
    else:
        check(lib().vidc_conv2d_plan(C.byref(d)), "conv plan")
    return d


class GenericArgs(C.Structure):
    _fields_ = [("p", C.c_void_p * 8), ("i", C.c_int32 * 16), ("f", C.c_float * 8)]


class _OpUnion(C.Union):
    _fields_ = [("conv", ConvDesc), ("g", GenericArgs)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("stream_id", C.c_int32), ("wait_mask", C.c_int32), ("reserved", C.c_int32),
                ("u", _OpUnion)]


class OpEntry(C.Structure):
    """vidc_op_entry (include/vidc.h): the entry point an op kind runs and the classes of its arguments."""
    _fields_ = [("_name", C.c_char_p), ("_classes", C.c_char_p)]
    name = property(lambda self: self._name.decode())
    classes = property(lambda self: self._classes.decode())


_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
# name -> (restype, argtypes); every symbol include/vidc.h declares
SIGNATURES = {
    "vidc_version": (C.c_int, []),
    "vidc_last_error": (C.c_char_p, []),
    "vidc_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, _i]),
    "vidc_warp2dof_params": (C.c_int, [_vp, _vp, _i, _f, _f, _f, _f, _vp, _i, _i, _vp, _vp]),
    "vidc_warp2dof_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp]),
    "vidc_warp2dof_inv_rot_norm": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _i, _vp]),
    "vidc_warp2dof_fwd_backward": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp]),
    "vidc_warp2dof_inv_rot_norm_backward": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _i, _vp]),
    "vidc_warp2dof_fwd_mode": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _i, _i, _vp]),
    "vidc_warp2dof_fwd_mode_backward": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _i, _i, _vp]),
    "vidc_warp2dof_grids": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp]),
    "vidc_affine_act_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_stem_conv3x3s2_backward_data": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_pack_conv_weight": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vidc_split_bf16x3": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _vp]),
    "vidc_pack_conv_weight_bf16x3": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vidc_pack_conv_weight_bf16": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vidc_quant_mxfp8": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _i, _vp]),
    "vidc_pack_conv_weight_mxfp8": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vidc_conv2d_bn_act": (C.c_int, [C.POINTER(ConvDesc), _vp]),
    "vidc_conv2d_workspace_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "vidc_conv2d_plan": (C.c_int, [C.POINTER(ConvDesc)]),
    "vidc_conv_tile_info": (C.c_int, [_i, C.POINTER(TileInfo)]),
    "vidc_train_scratch_bytes": (C.c_size_t, [C.c_longlong, _i]),
    "vidc_bn_train_forward": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "vidc_bn_train_forward_add": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "vidc_bn_train_forward_stats": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "vidc_bn_train_backward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_bn_train_backward_t": (C.c_int, [_vp, _vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "vidc_bn_eval_forward_add": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _i, _vp, _i, _vp]),
    "vidc_bn_eval_backward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "vidc_colsum": (C.c_int, [_vp, C.c_longlong, _i, _i, _vp, _vp, _vp]),
    "vidc_add_rows": (C.c_int, [_vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp]),
    "vidc_add_rows_bf16": (C.c_int, [_vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_relu_backward": (C.c_int, [_vp, _vp, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp]),
    "vidc_maxpool3x3s2_backward": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_upsample_bilinear_ac_backward": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_head_backward_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "vidc_head_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_masked_l1_loss": (C.c_int, [_vp, _vp, C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp]),
    "vidc_normal_l1_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_normal_l1_loss": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_dropout2d_mask": (C.c_int, [_vp, _i, _i, _f, C.c_ulonglong, C.c_ulonglong, _vp]),
    "vidc_scale_image_channels": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vidc_normalize_nchw_backward": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "vidc_depth_l1_loss_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_depth_l1_loss": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_head_backward_multi_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "vidc_head_backward_multi": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_clock_stamp": (C.c_int, [_vp, _vp]),
    "vidc_adam_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_longlong, _f, _f, _f, _f, _i, _vp]),
    "vidc_grad_sqnorm_scratch_bytes": (C.c_size_t, [C.c_longlong]),
    "vidc_grad_sqnorm": (C.c_int, [_vp, C.c_longlong, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "vidc_grad_accumulate": (C.c_int, [_vp, _vp, C.c_longlong, _i, _vp]),
    "vidc_optimizer_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_longlong, _f, _f, _f, _f, _i, _i, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_train_bn_fold": (C.c_int, [_i]),
    "vidc_grad_narrow_bf16": (C.c_int, [_vp, _vp, C.c_longlong, _vp]),
    "vidc_grad_widen_bf16": (C.c_int, [_vp, _vp, C.c_longlong, _vp]),
    "vidc_pack_conv_weight_dgrad": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vidc_cast_bf16": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _vp]),
    "vidc_host_mt19937_permutation_prefix": (C.c_int, [_vp, _vp, C.c_longlong, _i, _vp, _vp]),
    "vidc_pack_item_blocks": (C.c_longlong, [_i, _i, _i, _i, _i]),
    "vidc_pack_conv_weights_batched": (C.c_int, [_vp, _i, C.c_longlong, _vp]),
    "vidc_pack_conv_weights_one": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vidc_zero_stuff": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_conv_wgrad_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "vidc_conv_wgrad": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_im2col_transposed": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_conv_wgrad_dilated_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "vidc_conv_wgrad_dilated": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_conv_wgrad_bf16_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "vidc_conv_wgrad_bf16": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_im2col_transposed_dilated": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_wgrad_permute": (C.c_int, [_vp, _vp, _i, _i, _i, _vp]),
    "vidc_transpose_bf16": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _vp]),
    "vidc_im2col_transposed_bf16": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_stem_wgrad_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "vidc_stem_wgrad": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_winograd_tiles": (C.c_int, [_i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vidc_winograd_weight_transform": (C.c_int, [_vp, _vp, _i, _i, _i, _vp]),
    "vidc_winograd_weight_pack_fused": (C.c_int, [_vp, _vp, _i, _i, _vp]),
    "vidc_winograd_input_transform": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_winograd_output_transform": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_stem_conv3x3s2": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "vidc_stem_conv3x3s2_warped": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _f, _f, _i, _vp]),
    "vidc_maxpool3x3s2": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_upsample_bilinear_ac": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "vidc_avgpool2d": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_avgpool2d_backward": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_normalize_nchw": (C.c_int, [_vp, _vp, _i, _i, _i, _vp]),
    "vidc_head_conv1x1_upsample": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_plane_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_plane_ransac_normal": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "vidc_plane_offset": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "vidc_plane_offset_dense": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_plane_project_depth": (C.c_int, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "vidc_plane_info_count": (C.c_int, [_i, _i]),
    "vidc_plane_finalize": (C.c_int, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vidc_plane_block": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vidc_enrich_scatter": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "vidc_enrich_scatter_from": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "vidc_resize_coeffs": (C.c_int, [_i, _i, _vp, _vp, _i, C.POINTER(C.c_int)]),
    "vidc_resize_bilinear_u8_to_chw": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "vidc_rasterize_sparse_depth": (C.c_int, [_vp, _vp, _i, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _i, _i, _vp]),
    "vidc_nearest_table": (C.c_int, [_i, _i, _vp]),
    "vidc_resize_nearest_u16_depth": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, C.c_float, _vp]),
    "vidc_u8_decode_chw": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vidc_rasterize_pixel_tracks_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_rasterize_pixel_tracks": (C.c_int, [_vp, _vp, _i, _i, C.c_double, _vp, _vp, _i, _i, _vp, _vp]),
    "vidc_nonzero_compact_scratch_bytes": (C.c_size_t, [_i, _i]),
    "vidc_nonzero_compact": (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "vidc_sparse_sample_scatter": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "vidc_resize_nearest_u16_depth_range": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, C.c_float, C.c_float, C.c_float, _vp]),
    "vidc_depth_metrics_scratch_bytes": (C.c_size_t, [C.c_longlong]),
    "vidc_depth_metrics": (C.c_int, [_vp, _vp, C.c_longlong, _vp, _i, _vp, _vp]),
    "vidc_depth_to_mm_u32": (C.c_int, [_vp, _vp, C.c_longlong, _vp]),
    "vidc_normal_metrics": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "vidc_hist_u16": (C.c_int, [_vp, C.c_longlong, _i, _vp, _vp]),
    "vidc_png_file_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_png_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "vidc_png_encode": (C.c_int, [_vp, _i, _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
    "vidc_png_deflate_max_file_bytes": (C.c_size_t, [_i, _i, _i]),
    "vidc_png_deflate_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "vidc_png_encode_deflate": (C.c_int, [_vp, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp, _vp, _vp]),
    "vidc_nms_scratch_bytes": (C.c_size_t, [_i]),
    "vidc_nms": (C.c_int, [_vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "vidc_nms_segmented_scratch_bytes": (C.c_size_t, [_i, _i]),
    "vidc_nms_segmented": (C.c_int, [_vp, _vp, _vp, _i, _i, _f, _i, _i, _vp, _vp, _vp, _vp]),
    "vidc_roi_align_forward": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "vidc_det_stem_im2col": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp]),
    "vidc_upsample_nearest2x": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_mask_scale": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "vidc_rpn_topk_decode": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, C.c_longlong, _vp]),
    "vidc_rpn_topk_decode_levels": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_longlong, _vp]),
    "vidc_rpn_select": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "vidc_roi_align_fpn": (C.c_int, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "vidc_det_candidates": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "vidc_det_select": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "vidc_mask_paste": (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "vidc_instance_map_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "vidc_instance_map": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp]),
    "vidc_op_info": (C.c_int, [_i, C.POINTER(OpEntry)]),
    "vidc_program_create": (C.c_int, [C.POINTER(Op), _i, C.POINTER(_vp)]),
    "vidc_program_run": (C.c_int, [_vp, _vp]),
    "vidc_program_capture": (C.c_int, [_vp, _vp]),
    "vidc_program_launch": (C.c_int, [_vp, _vp]),
    "vidc_program_run_range": (C.c_int, [_vp, _vp, _i, _i]),
    "vidc_program_capture_range": (C.c_int, [_vp, _vp, _i, _i, _i]),
    "vidc_program_launch_segment": (C.c_int, [_vp, _vp, _i]),
    "vidc_program_time": (C.c_int, [_vp, _vp, _i, _i, _f32p, _f32p]),
    "vidc_program_destroy": (C.c_int, [_vp]),
}

_lib = None


def build(force=False, verbose=False):
    """Compile libvidc.so in-tree: hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".def", ".map")) or f == "Makefile"]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "vidc.h"))
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cmd = ["make", "-C", CSRC, "-j%d" % min(8, os.cpu_count() or 1)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("building libvidc.so failed (hipcc, gfx950)")
    return LIB_PATH


def lib():
    """The loaded library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libvidc.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`. "
                               "There is no CPU/eager fallback for the HIP path." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)     # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if L.vidc_version() != 1:
            raise RuntimeError("libvidc.so ABI version mismatch")
        _lib = L
    return _lib


_TILE_TABLES = ("TILE_INFO", "TILE_COUNT", "TILE_NAMES", "MXFP8_TILES", "BF16_TILES", "TILE_WINO4_FUSED")


def __getattr__(name):
    """The tile tables: id -> vidc_tile_info, id -> name, the number of ids, the ids with an MXFP8 / a plain-bf16 instance, the fused Winograd
    tile.  Read from the library's own table (csrc/conv_tiles.def) on first use, then module attributes: no copy is written down here."""
    if name not in _TILE_TABLES:
        raise AttributeError("module %r has no attribute %r" % (__name__, name))
    info, ti = {}, TileInfo()
    while lib().vidc_conv_tile_info(len(info), C.byref(ti)) == 0:      # (fails past the last id)
        info[len(info)], ti = ti, TileInfo()
    globals().update(TILE_INFO=info, TILE_COUNT=len(info), TILE_NAMES={t: ti.name for t, ti in info.items()},
                     MXFP8_TILES=tuple(t for t, ti in info.items() if ti.precisions >> PREC_MXFP8 & 1),
                     BF16_TILES=tuple(t for t, ti in info.items() if ti.precisions >> PREC_BF16 & 1),
                     TILE_WINO4_FUSED=next(t for t, ti in info.items() if ti.kind == TILE_KIND_WINOGRAD))
    return globals()[name]


# ---- the slot rule of vidc_generic_args (include/vidc.h) is written in pack_op / op_args and nowhere else in Python -------------------
_op_classes = {}


def op_classes(kind):
    """The argument classes of an op kind's entry point, one char per parameter without the stream (vidc_op_info)."""
    if kind not in _op_classes:
        e = OpEntry()
        check(lib().vidc_op_info(kind, C.byref(e)), "op_info")
        _op_classes[kind] = e.classes
    return _op_classes[kind]


def pack_op(op, kind, args):
    """op.kind = kind and op.u.g = `args`, the arguments of the kind's entry point in the header's declaration order without the stream:
    a pointer (an int, or None) takes the next p slot, an int the next i slot, a float the next f slot, a long long the next two i slots
    (low word, then high word); the other slots are zero.  Raises on a wrong argument count, a non-integer where a pointer or an int is
    due, an int outside int32 and an entry that needs more slots than there are."""
    if kind == OP_CONV:
        raise ValueError("a conv op carries its descriptor (op.u.conv), not argument slots")
    classes = op_classes(kind)
    if len(args) != len(classes):
        raise ValueError("op kind %d takes %d arguments (%s), got %d" % (kind, len(classes), classes, len(args)))
    slots = {"p": [], "i": [], "f": []}
    for c, v in zip(classes, args):
        if c == "f":
            slots["f"].append(float(v))
            continue
        v = 0 if v is None and c == "p" else operator.index(v)      # (TypeError for a float or a tensor)
        if c == "p":
            slots["p"].append(v)
        elif c == "l":
            slots["i"] += [v & 0xFFFFFFFF, v >> 32 & 0xFFFFFFFF]
        elif -1 << 31 <= v < 1 << 31:
            slots["i"].append(v)
        else:
            raise ValueError("op kind %d: %d does not fit an int" % (kind, v))
    g = GenericArgs()
    for c, vals in slots.items():
        arr = getattr(g, c)
        if len(vals) > len(arr):
            raise ValueError("op kind %d needs %d %s slots of %d" % (kind, len(vals), c, len(arr)))
        for j, v in enumerate(vals):
            arr[j] = v
    op.kind, op.u.g = kind, g
    return op


def op_args(op):
    """The inverse of pack_op: the arguments of a packed op in declaration order (a null pointer as 0)."""
    g, n, out = op.u.g, {"p": 0, "i": 0, "f": 0}, []
    for c in op_classes(op.kind):
        k = "i" if c == "l" else c
        v = getattr(g, k)[n[k]] or 0
        n[k] += 1
        if c == "l":
            v, n["i"] = (v & 0xFFFFFFFF) | g.i[n["i"]] << 32, n["i"] + 1
        out.append(v)
    return tuple(out)


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("libvidc %s failed (status %d): %s" % (what, rc, lib().vidc_last_error().decode()))


def ptr(t):
    """Raw device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


_raw_stream = None


def current_stream():
    """Raw hipStream_t of torch's current stream on the current device.  Called once per launch from Python: the private C accessors
    (no Stream object, no device-index resolution: ~0.3 us instead of ~7 us, 15 calls per frame in the stream modes) when this torch has
    them, torch.cuda.current_stream() otherwise."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        get_raw, get_dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        if get_raw is not None and get_dev is not None:
            _raw_stream = lambda: get_raw(get_dev())          # noqa: E731
        else:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
    return _raw_stream()
