"""`torch.ops.vidc.*`: the C entry points of libvidc.so registered as PyTorch custom operators (north_star: "exposed as
custom torch ops through a thin C-ABI extension").

Every operator is registered for the GPU dispatch key only (`device_types="cuda"`, which is HIP on ROCm): calling one with
CPU tensors raises PyTorch's "no kernel for backend CPU" error -- there is deliberately no CPU implementation.  Shape
functions (`register_fake`) are provided so the operators can be traced/exported; they allocate nothing on a device.

The networks' inference does not dispatch through these (a network is ONE `vidc_program_run`/hipGraph replay, engine.py); the operators are the
per-op surface for callers that compose the kernels with other PyTorch code, and what the three networks' `forward_autograd` (with
networks/autograd_blocks.py) are composed of.  OPS lists every name; the tuples at the end of the file group them by the layer that added them.

Inference surface (differentiable where the Autograd section says so):

    torch.ops.vidc.warp2dof_fwd(x, g, a, fx, fy, cx, cy, align_corners)      warping_2dof_alignment.py:108-156
    torch.ops.vidc.warp2dof_inv_rot_norm(x, g, a, fx, fy, cx, cy, align_corners, normalize)   :216-255 (+ surface_normal.py:170)
    torch.ops.vidc.warp2dof_fwd_mode(x, g, a, fx, fy, cx, cy, align_corners, mode, rotate)    :108-156 with interp_mode (0 bilinear, 1 nearest, 2 bicubic); rotate: :258-290
    torch.ops.vidc.warp2dof_grids(g, a, fx, fy, cx, cy, W, H) -> (C_R_Cg, grid, inv_grid)     :158-214 (not differentiable)
    torch.ops.vidc.plane_ransac_normal(normals, ids, slots, hyp_pix)          main.py:38-62 (+ the write-back of :157)
    torch.ops.vidc.plane_offset(homo, depth, slots, inlier_mask, counts, scratch)       main.py:68-101, 162-173
    torch.ops.vidc.plane_project_depth(homo, slots, inlier_mask, scratch, records, plane_depth)   main.py:110-127
    torch.ops.vidc.plane_finalize(depth, plane_depth, records)                main.py:186-187 + the candidate counts of :287-289
    torch.ops.vidc.enrich_scatter(plane_depth, sparse_depth, sub, sub_offsets, chunk_base)        main.py:286, 290-294
(the host-side draws that feed the plane operators -- np.random.permutation / randint in the reference's order -- are plane.draw_normal_hypotheses
and plane.draw_enrichment; plane.PlaneBlock is the composition the pipeline uses)

Differentiable convs and glue (with the two warps: backward operators in BACKWARD_OPS; DORN_OPS / DORN_BACKWARD_OPS are the two operators of
SurfaceNormalDORN's scene-understanding module and their backwards):

    torch.ops.vidc.conv2d_bn_act(x_nhwc, w_oihw, scale, shift, stride, pad, relu, precision)  Conv2d+BatchNorm2d(eval)+ReLU
    torch.ops.vidc.conv3x3_winograd(x_nhwc, w_oihw, scale, shift, m, relu, precision)         the 3x3 / stride-1 layers as Winograd F(m x m, 3x3)
    torch.ops.vidc.conv2d_dilated_bn_act(x_nhwc, w_oihw, scale, shift, pad, dilation, relu, precision)   surface_normal_dorn.py:45-68 (the ASPP branches)
    torch.ops.vidc.stem_conv3x3s2(x_nchw, w_oihw, relu)                       surface_normal.py:36 (conv1_1, no BN)
    torch.ops.vidc.maxpool3x3s2(x_nhwc)                                       torchvision ResNet.maxpool
    torch.ops.vidc.avgpool2d(x_nhwc, kh, kw, sh, sw, ph, pw)                  surface_normal_dorn.py:10 (nn.AvgPool2d, count_include_pad=True)
    torch.ops.vidc.upsample_bilinear_ac(x_nhwc, Ho, Wo, relu)                 nn.UpsamplingBilinear2d (align_corners=True)
    torch.ops.vidc.head_conv1x1_upsample(x_nhwc, w, bias, pad, Ho, Wo, relu)  depth_completion.py:141-147 / surface_normal.py:140-145

Train-mode operators (TRAIN_OPS / TRAIN_BACKWARD_OPS, added for SurfaceNormalDORN; NET_TRAIN_OPS / NET_TRAIN_BACKWARD_OPS, added for ModifiedFPN and
SurfaceNormalPrediction):

    torch.ops.vidc.batch_norm_train(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None) -> (y, save_mean, save_rstd)
    torch.ops.vidc.batch_norm_eval(x_nhwc, gamma, beta, running_mean, running_var, eps, relu, residual=None) -> y     a frozen BatchNorm2d (FROZEN_BN_OPS)
    torch.ops.vidc.dropout2d(x_nhwc, p, seed, offset) -> (y, keep)           nn.Dropout2d in train() mode, Philox4x32-10 per (image, channel)
    torch.ops.vidc.scale_image_channels(x_nhwc, keep)                        y = x * keep[b][c]: Dropout2d for a given keep table; its own backward
    torch.ops.vidc.normalize_nchw(x)                                         F.normalize(x, dim=1), surface_normal_dorn.py:154
    torch.ops.vidc.feature_mask_scale(x_nhwc, image_nchw)                    surface_normal.py:151-162 (the use_mask multiply; image gets no gradient)
    torch.ops.vidc.add_rows(a, b, relu)                                      z1 + z2 + z3 + z4 of both decoders

batch_norm_train is nn.BatchNorm2d in train() mode (+ residual, + ReLU) on the trainers' kernels, updates the running statistics in place, and reads
x in place when it is a channel slice.  batch_norm_eval is nn.BatchNorm2d in eval() mode (+ residual, + ReLU) inside a training step -- what
forward_autograd runs for a BatchNorm module that is itself in eval() mode: the running statistics are read and never written, gradients go to x,
gamma, beta and residual, and its backward (vidc_bn_eval_backward) launches the per-channel reduction only when gamma or beta asks for a gradient
(x is saved only then) and writes dx only when x does.  feature_mask_scale is vidc_mask_scale and its own backward; add_rows is vidc_add_rows, its backward vidc_relu_backward.

Losses (normal_l1_loss in TRAIN_OPS, depth_l1_loss in NET_TRAIN_OPS; both registered the same way, _register_l1_loss_backward):

    torch.ops.vidc.normal_l1_loss(pred, normal_gt, mask, normalize_prediction) -> (loss, count, angle)     network_run.py:181-189
    torch.ops.vidc.depth_l1_loss(pred, depth_gt) -> (loss, count, ratios)    network_run.py:165-179 (+ GetDepthPrintableRatios, :72-82: depth_printable_ratios)

Each is one kernel call (vidc_normal_l1_loss of csrc/sn_train.hip; vidc_depth_l1_loss of csrc/net_train.hip: loss, its gradient, the valid count and the
five ratio counts, fp64 sums in a fixed two-level order) that writes the loss's gradient beside the sums: `*_with_grad` returns it as a fourth output,
and the loss operator is the first three outputs of that.

Autograd.  The warps, the convs, the glue, the train-mode operators and the losses are differentiable: each has a backward registered with
`torch.library.register_autograd` (batch_norm_train, which mutates its running statistics, through an autograd.Function), and each backward formula is
itself a custom operator (`torch.ops.vidc.*_backward`, listed in the *_BACKWARD_OPS tuples) with a shape function, or the forward operator applied to
the gradient (scale_image_channels, which is also dropout2d's backward, and feature_mask_scale), built from HIP kernels only -- the warp adjoints of
csrc/warp.hip, vidc_affine_act_backward + zero-stuffing + the conv kernel on data-gradient weights + vidc_conv_wgrad for the convs (precision 0 and 1; Winograd forwards share the
direct form's backward; the data gradient runs in exact fp32 except behind a Winograd forward at precision 1, where it runs in bf16x3 like
the forward; inside `grad_precision(2)` both conv gradients of every conv operator run in plain bf16 instead -- the data gradient on the conv
kernel at precision 2, the weight gradient on vidc_conv_wgrad_bf16 -- where ops.conv_backward_data_precision / conv_backward_weight_precision
allow it, while dc, dscale, dshift and the forward keep their arithmetic), the backward kernels of csrc/train.hip for the glue, batch_norm_train and normalize_nchw.  Gradients flow to images / activations, conv weights, the
folded scale / shift and the head's bias; only those `ctx.needs_input_grad` asks for are computed, and nothing is saved when gradients are
disabled.  `gravity` / `aligned` get no gradient (the warp record is built with cosf / atan2f / bbox min-max) and precision 3 (MXFP8) has no
backward: requesting either raises.  The dilated conv's backward is the direct form's with stride 1: the data gradient is the conv kernel on
the data-gradient weights with the same dilation and pad' = dilation * (k - 1) - pad, the weight gradient vidc_conv_wgrad_dilated; avgpool2d's
is vidc_avgpool2d_backward.  The head's backward covers up to four output channels with pad 0 or 1 (vidc_head_backward_multi on B * Cout
one-channel planes: the depth head, surface_normal.py:143 and surface_normal_dorn.py:74-75).  A loss's backward is dpred * grad_loss.  Double backward
is not supported.  The plane operators (`plane_*`, `enrich_scatter`) stay non-differentiable: they are RANSAC decisions and index scatters.
"""
import contextlib
import threading
from typing import Optional, Tuple

import torch

from . import ops as _ops
from .networks.warping_2dof_alignment import Warping2DOFAlignment

_DEV = "cuda"


_grad_state = threading.local()


def current_grad_precision():
    """The arithmetic of the conv gradients that a conv forward records for its backward: 0 (fp32; the default) or 2 (plain bf16)."""
    return getattr(_grad_state, "precision", 0)


@contextlib.contextmanager
def grad_precision(p):
    """Context manager: conv operators whose FORWARD runs inside record `p` as the arithmetic of their data and weight gradients.  0: today's
    backward (exact fp32; bf16x3 data gradient behind a Winograd forward at precision 1).  2: plain bf16 operands with fp32 accumulation
    (conv2d_bn_act_backward).  Re-entrant; the previous value is restored on exit.  The forward's own `precision` is a separate knob."""
    if p not in (0, 2):
        raise RuntimeError("grad_precision: the gradient arithmetic is 0 (fp32) or 2 (plain bf16), got %r" % (p,))
    previous = current_grad_precision()
    _grad_state.precision = p
    try:
        yield
    finally:
        _grad_state.precision = previous


def _warper(x, fx, fy, cx, cy, align_corners):
    return Warping2DOFAlignment(fx, fy, cx, cy, align_corners=align_corners, device=x.device)


@torch.library.custom_op("vidc::warp2dof_fwd", mutates_args=(), device_types=_DEV)
def warp2dof_fwd(x: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                 align_corners: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Cg_H_C (B,3,3), warped x (B,C,H,W)) -- Warping2DOFAlignment.warp_with_gravity_center_aligned."""
    h, y = _warper(x, fx, fy, cx, cy, align_corners).warp_with_gravity_center_aligned(x, gravity, aligned)
    return h, y


@warp2dof_fwd.register_fake
def _(x, gravity, aligned, fx, fy, cx, cy, align_corners):
    return x.new_empty((x.shape[0], 3, 3)), torch.empty_like(x)


@torch.library.custom_op("vidc::warp2dof_inv_rot_norm", mutates_args=(), device_types=_DEV)
def warp2dof_inv_rot_norm(x: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                          align_corners: bool, normalize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Cg_H_C, R^T-rotated inverse-warped normals [unit length if normalize]) -- inverse_warp_normal_image_with_gravity_center_aligned."""
    h, z = _warper(x, fx, fy, cx, cy, align_corners).inverse_warp_normal_image_with_gravity_center_aligned(x, gravity, aligned,
                                                                                                            normalize=normalize)
    return h, z


@warp2dof_inv_rot_norm.register_fake
def _(x, gravity, aligned, fx, fy, cx, cy, align_corners, normalize):
    return x.new_empty((x.shape[0], 3, 3)), torch.empty_like(x)


def _pack_for(precision):
    """The weight packing of a conv precision (conv2d_bn_act's docstring); any other value packs exact fp32."""
    return {1: _ops.pack_conv_weight_bf16x3, 2: _ops.pack_conv_weight_bf16, 3: _ops.pack_conv_weight_mxfp8}.get(precision, _ops.pack_conv_weight)


@torch.library.custom_op("vidc::conv2d_bn_act", mutates_args=(), device_types=_DEV)
def conv2d_bn_act(x_nhwc: torch.Tensor, w_oihw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int, pad: int,
                  relu: bool, precision: int) -> torch.Tensor:
    """relu?(conv(x, w) * scale + shift) on NHWC activations; scale/shift = the folded bias + eval-mode BatchNorm
    (engine.fold_bn); precision 0 = exact fp32 MFMA, 1 = bf16x3, 2 = plain bf16 (input and weights rounded to bf16, fp32 accumulation;
    Cin % 64 == 0), 3 = MXFP8: the fp32 input is quantised and the weights packed block-scaled; the output is fp32 (vidc_conv_precision)."""
    return _ops.conv2d_bn_act(x_nhwc, _pack_for(precision)(w_oihw), scale, shift, w_oihw.shape[2], w_oihw.shape[3], stride=stride, pad=pad,
                              relu1=relu, precision=precision)


@conv2d_bn_act.register_fake
def _(x_nhwc, w_oihw, scale, shift, stride, pad, relu, precision):
    B, H, W, _c = x_nhwc.shape
    co, _ci, kh, kw = w_oihw.shape
    return x_nhwc.new_empty((B, (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1, co))


@torch.library.custom_op("vidc::conv2d_dilated_bn_act", mutates_args=(), device_types=_DEV)
def conv2d_dilated_bn_act(x_nhwc: torch.Tensor, w_oihw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, pad: int, dilation: int, relu: bool,
                          precision: int) -> torch.Tensor:
    """conv2d_bn_act for a dilated conv of stride 1 (the ASPP branches, surface_normal_dorn.py:45-68: Conv2d(2048, 512, 3, padding=d, dilation=d) +
    BatchNorm2d(eval) + ReLU, d = 6 / 12 / 18): tap (kh, kw) reads x[oy - pad + kh * dilation, ox - pad + kw * dilation]; precision as there."""
    return _ops.conv2d_bn_act(x_nhwc, _pack_for(precision)(w_oihw), scale, shift, w_oihw.shape[2], w_oihw.shape[3], stride=1, pad=pad, relu1=relu,
                              precision=precision, dilation=dilation)


@conv2d_dilated_bn_act.register_fake
def _(x_nhwc, w_oihw, scale, shift, pad, dilation, relu, precision):
    B, H, W, _c = x_nhwc.shape
    co, _ci, kh, kw = w_oihw.shape
    return x_nhwc.new_empty((B, H + 2 * pad - dilation * (kh - 1), W + 2 * pad - dilation * (kw - 1), co))


@torch.library.custom_op("vidc::conv3x3_winograd", mutates_args=(), device_types=_DEV)
def conv3x3_winograd(x_nhwc: torch.Tensor, w_oihw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, m: int, relu: bool,
                     precision: int) -> torch.Tensor:
    """relu?(conv3x3(x, w, stride 1, pad 1) * scale + shift) as Winograd F(m x m, 3x3), m = 2 or 4: input transform, the a*a
    transform-domain GEMMs as one grouped launch of the MFMA conv kernel, output transform with the epilogue (csrc/winograd.hip);
    the form the networks' 3x3 layers run in where the measured table says so.  precision as in conv2d_bn_act."""
    return _ops.conv3x3_winograd(x_nhwc, [w_oihw], scale.reshape(1, -1), shift.reshape(1, -1), m, relu1=relu, precision=precision)


@conv3x3_winograd.register_fake
def _(x_nhwc, w_oihw, scale, shift, m, relu, precision):
    B, H, W, _c = x_nhwc.shape
    return x_nhwc.new_empty((B, H, W, w_oihw.shape[0]))


@torch.library.custom_op("vidc::stem_conv3x3s2", mutates_args=(), device_types=_DEV)
def stem_conv3x3s2(x_nchw: torch.Tensor, w_oihw: torch.Tensor, relu: bool) -> torch.Tensor:
    return _ops.stem_conv3x3s2(x_nchw, w_oihw, relu=relu)


@stem_conv3x3s2.register_fake
def _(x_nchw, w_oihw, relu):
    B, _c, H, W = x_nchw.shape
    return x_nchw.new_empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, w_oihw.shape[0]))


@torch.library.custom_op("vidc::maxpool3x3s2", mutates_args=(), device_types=_DEV)
def maxpool3x3s2(x_nhwc: torch.Tensor) -> torch.Tensor:
    return _ops.maxpool3x3s2(x_nhwc)


@maxpool3x3s2.register_fake
def _(x_nhwc):
    B, H, W, Cc = x_nhwc.shape
    return x_nhwc.new_empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc))


@torch.library.custom_op("vidc::avgpool2d", mutates_args=(), device_types=_DEV)
def avgpool2d(x_nhwc: torch.Tensor, kh: int, kw: int, sh: int, sw: int, ph: int, pw: int) -> torch.Tensor:
    """nn.AvgPool2d((kh, kw), (sh, sw), (ph, pw)) with count_include_pad=True on NHWC (FullImageEncoder.global_pooling, surface_normal_dorn.py:10)."""
    return _ops.avgpool2d(x_nhwc, (kh, kw), (sh, sw), (ph, pw))


@avgpool2d.register_fake
def _(x_nhwc, kh, kw, sh, sw, ph, pw):
    B, H, W, Cc = x_nhwc.shape
    return x_nhwc.new_empty((B, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1, Cc))


@torch.library.custom_op("vidc::upsample_bilinear_ac", mutates_args=(), device_types=_DEV)
def upsample_bilinear_ac(x_nhwc: torch.Tensor, out_h: int, out_w: int, relu: bool) -> torch.Tensor:
    return _ops.upsample_bilinear_ac(x_nhwc, (out_h, out_w), relu=relu)


@upsample_bilinear_ac.register_fake
def _(x_nhwc, out_h, out_w, relu):
    return x_nhwc.new_empty((x_nhwc.shape[0], out_h, out_w, x_nhwc.shape[3]))


@torch.library.custom_op("vidc::head_conv1x1_upsample", mutates_args=(), device_types=_DEV)
def head_conv1x1_upsample(x_nhwc: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pad: int, out_h: int, out_w: int,
                          relu: bool) -> torch.Tensor:
    """NCHW (B,Cout,out_h,out_w): 1x1 conv (+bias, zero padding `pad`) -> bilinear(align_corners=True) -> ReLU?"""
    return _ops.head_conv1x1_upsample(x_nhwc, w, bias, pad, (out_h, out_w), relu)[0]


@head_conv1x1_upsample.register_fake
def _(x_nhwc, w, bias, pad, out_h, out_w, relu):
    return x_nhwc.new_empty((x_nhwc.shape[0], w.shape[0], out_h, out_w))


# ---- plane block (csrc/plane.hip) ------------------------------------------------------------------------------------------------
from . import _lib as _L  # noqa: E402


def _st():
    return _L.current_stream()


@torch.library.custom_op("vidc::plane_ransac_normal", mutates_args=(), device_types=_DEV)
def plane_ransac_normal(normals: torch.Tensor, ids: torch.Tensor, slots: torch.Tensor, hyp_pix: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """normals (B,3,H,W) fp32 unit normals, ids (B,H,W) uint8 plane ids, slots (n,4) int32 = (image, id, hypothesis offset, count),
    hyp_pix int32 flat pixel indices of the hypotheses -> (inlier_mask (n,H*W) uint8, counts (n,300) int32, scratch uint8: the partial
    sums the next two stages read)."""
    B, _c, H, W = normals.shape
    n, HW = slots.shape[0], H * W
    lib = _L.lib()
    mask = torch.empty((n, HW), dtype=torch.uint8, device=normals.device)
    counts = torch.empty((n, _L.MAX_HYP), dtype=torch.int32, device=normals.device)
    scratch = torch.empty(lib.vidc_plane_scratch_bytes(n, B, HW), dtype=torch.uint8, device=normals.device)
    _L.check(lib.vidc_plane_ransac_normal(_L.ptr(normals.contiguous()), _L.ptr(ids.contiguous()), _L.ptr(slots.contiguous()), n,
                                          _L.ptr(hyp_pix.contiguous()), HW, _L.ptr(mask), _L.ptr(counts), _L.ptr(scratch), _st()), "plane_ransac_normal")
    return mask, counts, scratch


@plane_ransac_normal.register_fake
def _(normals, ids, slots, hyp_pix):
    B, _c, H, W = normals.shape
    n = slots.shape[0]
    nc = (H * W + 255) // 256
    return (normals.new_empty((n, H * W), dtype=torch.uint8), normals.new_empty((n, 300), dtype=torch.int32),
            normals.new_empty((n * nc * 9 * 4 + B * (H * W + 1) * 4 + 256,), dtype=torch.uint8))


@torch.library.custom_op("vidc::plane_offset", mutates_args=(), device_types=_DEV)
def plane_offset(homo: torch.Tensor, depth: torch.Tensor, slots: torch.Tensor, inlier_mask: torch.Tensor, counts: torch.Tensor,
                 scratch: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """homo (B,H,W,3), depth (B,1,H,W) sparse depth -> (records (n,16) fp32 [include/vidc.h], scratch passed on).  Planes with more than
    300 sparse points come back flagged (record[10] = -1): plane.PlaneBlock resolves them with the reference's host permutation."""
    B = homo.shape[0]
    n, HW = inlier_mask.shape
    sc = scratch.clone()
    rec = torch.empty((n, _L.PLANE_RECORD), dtype=torch.float32, device=homo.device)
    _L.check(_L.lib().vidc_plane_offset(_L.ptr(homo.contiguous()), _L.ptr(depth.contiguous()), _L.ptr(slots.contiguous()), n, B,
                                        _L.ptr(inlier_mask), _L.ptr(counts), HW, _L.ptr(sc), _L.ptr(rec), _st()), "plane_offset")
    return rec, sc


@plane_offset.register_fake
def _(homo, depth, slots, inlier_mask, counts, scratch):
    return homo.new_empty((inlier_mask.shape[0], 16)), torch.empty_like(scratch)


@torch.library.custom_op("vidc::plane_project_depth", mutates_args=(), device_types=_DEV)
def plane_project_depth(homo: torch.Tensor, slots: torch.Tensor, inlier_mask: torch.Tensor, scratch: torch.Tensor, records: torch.Tensor,
                        plane_depth: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """generate_depth_from_plane for every slot: (plane_depth with the valid planes written in, records with [10], [11] filled)."""
    n, HW = inlier_mask.shape
    out, rec, sc = plane_depth.contiguous().clone(), records.clone(), scratch.clone()
    _L.check(_L.lib().vidc_plane_project_depth(_L.ptr(homo.contiguous()), _L.ptr(slots.contiguous()), n, _L.ptr(inlier_mask), HW, _L.ptr(sc),
                                               _L.ptr(rec), _L.ptr(out), _st()), "plane_project_depth")
    return out, rec


@plane_project_depth.register_fake
def _(homo, slots, inlier_mask, scratch, records, plane_depth):
    return torch.empty_like(plane_depth), torch.empty_like(records)


@torch.library.custom_op("vidc::plane_finalize", mutates_args=(), device_types=_DEV)
def plane_finalize(depth: torch.Tensor, plane_depth: torch.Tensor, records: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(plane_depth with the original sparse depths restored (main.py:186-187), info int32: per 256-pixel chunk the number of
    plane_depth > 0 pixels of every image, then the number of flagged slots)."""
    B = depth.shape[0]
    HW = depth.numel() // B
    out = plane_depth.contiguous().clone()
    info = torch.empty(_L.lib().vidc_plane_info_count(B, HW), dtype=torch.int32, device=depth.device)
    _L.check(_L.lib().vidc_plane_finalize(_L.ptr(depth.contiguous()), _L.ptr(out), B, HW, _L.ptr(records.contiguous()), records.shape[0],
                                          _L.ptr(info), _st()), "plane_finalize")
    return out, info


@plane_finalize.register_fake
def _(depth, plane_depth, records):
    B = depth.shape[0]
    HW = depth.numel() // B
    return torch.empty_like(plane_depth), depth.new_empty((B * ((HW + 255) // 256) + 1,), dtype=torch.int32)


@torch.library.custom_op("vidc::enrich_scatter", mutates_args=(), device_types=_DEV)
def enrich_scatter(plane_depth: torch.Tensor, sparse_depth: torch.Tensor, sub: torch.Tensor, sub_offsets: torch.Tensor,
                   chunk_base: torch.Tensor) -> torch.Tensor:
    """clone(sparse_depth) with the sub[]-th nonzeros (row-major) of plane_depth copied in, per image (main.py:286-294)."""
    B = sparse_depth.shape[0]
    HW = sparse_depth.numel() // B
    out = torch.empty_like(sparse_depth, memory_format=torch.contiguous_format)
    _L.check(_L.lib().vidc_enrich_scatter_from(_L.ptr(plane_depth.contiguous()), _L.ptr(sparse_depth.contiguous()), _L.ptr(sub.contiguous()),
                                               _L.ptr(sub_offsets.contiguous()), _L.ptr(chunk_base.contiguous()), B, HW, _L.ptr(out), _st()),
             "enrich_scatter")
    return out


@enrich_scatter.register_fake
def _(plane_depth, sparse_depth, sub, sub_offsets, chunk_base):
    return torch.empty_like(sparse_depth)


# ---- autograd: backward operators + their registration ----------------------------------------------------------------------------
def _none_if_empty(t):
    return t if t.numel() else None


def _no_geometry_grad(ctx, what, i_gravity, i_aligned):
    if ctx.needs_input_grad[i_gravity] or ctx.needs_input_grad[i_aligned]:
        raise RuntimeError("torch.ops.vidc.%s: gravity / aligned are not differentiable (the warp record is built with cosf / atan2f / bbox "
                           "min-max); detach them" % what)


def _register_warp_autograd(name, backward_op, n_args, saves_x=False):
    """The autograd formula of warp operator `name` -- (x, gravity, aligned, n_args plain arguments) -> (Cg_H_C, image): the gradient of the image
    through torch.ops.vidc.<backward_op>(grad, gravity, aligned, *arguments), none for anything else.  saves_x: the backward operator takes x in
    front, which is kept only if the last argument (normalize) is set -- the linear form reads no x and gets the gradient in its place."""
    def setup(ctx, inputs, output):
        x, gravity, aligned = inputs[:3]
        _no_geometry_grad(ctx, name, 1, 2)
        ctx.args = tuple(inputs[3:])
        assert len(ctx.args) == n_args
        saved = (gravity, aligned)
        if saves_x:
            saved = (x if ctx.args[-1] else x.new_empty(0),) + saved      # (the linear form reads no x)
        ctx.save_for_backward(*saved)

    def backward(ctx, _grad_h, grad):
        *x, gravity, aligned = ctx.saved_tensors
        if x and not x[0].numel():
            x = [grad]
        return (getattr(torch.ops.vidc, backward_op)(*x, grad, gravity, aligned, *ctx.args),) + (None,) * (2 + n_args)

    torch.library.register_autograd("vidc::" + name, backward, setup_context=setup)


@torch.library.custom_op("vidc::warp2dof_fwd_backward", mutates_args=(), device_types=_DEV)
def warp2dof_fwd_backward(dy: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                          align_corners: bool) -> torch.Tensor:
    """dx of warp2dof_fwd: the transposed bilinear gather (vidc_warp2dof_fwd_backward)."""
    wp = _warper(dy, fx, fy, cx, cy, align_corners)
    assert tuple(dy.shape[-2:]) == (wp.H, wp.W)
    return _ops.warp2dof_fwd_backward(dy, wp._params(gravity, aligned), cx, cy, align_corners)


@warp2dof_fwd_backward.register_fake
def _(dy, gravity, aligned, fx, fy, cx, cy, align_corners):
    return torch.empty_like(dy)


_register_warp_autograd("warp2dof_fwd", "warp2dof_fwd_backward", 5)


@torch.library.custom_op("vidc::warp2dof_inv_rot_norm_backward", mutates_args=(), device_types=_DEV)
def warp2dof_inv_rot_norm_backward(x: torch.Tensor, dz: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float,
                                   cx: float, cy: float, align_corners: bool, normalize: bool) -> torch.Tensor:
    """dx of warp2dof_inv_rot_norm through normalize, rotation and gather (vidc_warp2dof_inv_rot_norm_backward)."""
    wp = _warper(x, fx, fy, cx, cy, align_corners)
    assert tuple(x.shape[-2:]) == (wp.H, wp.W) and x.shape == dz.shape
    return _ops.warp2dof_inv_rot_norm_backward(x, dz, wp._params(gravity, aligned), cx, cy, align_corners, normalize)


@warp2dof_inv_rot_norm_backward.register_fake
def _(x, dz, gravity, aligned, fx, fy, cx, cy, align_corners, normalize):
    return torch.empty_like(x)


_register_warp_autograd("warp2dof_inv_rot_norm", "warp2dof_inv_rot_norm_backward", 6, saves_x=True)


# ---- the forward warp in grid_sample's three interpolation modes (WARP_MODE_OPS) --------------------------------------------------------------
@torch.library.custom_op("vidc::warp2dof_fwd_mode", mutates_args=(), device_types=_DEV)
def warp2dof_fwd_mode(x: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                      align_corners: bool, mode: int, rotate: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Cg_H_C (B,3,3), warped x (B,C,H,W)) in interpolation mode 0 bilinear / 1 nearest / 2 bicubic -- warp_with_gravity_center_aligned(interp_mode);
    with rotate (C == 3) the warped image is rotated by Cg_R_C per pixel -- warp_normal_image_with_gravity_center_aligned."""
    wp = _warper(x, fx, fy, cx, cy, align_corners)
    assert tuple(x.shape[-2:]) == (wp.H, wp.W) and x.dim() == 4
    p = wp._params(gravity, aligned)
    return p[:, 0:9].reshape(x.shape[0], 3, 3).clone(), _ops.warp2dof_fwd_mode(x, p, cx, cy, align_corners, mode, rotate)


@warp2dof_fwd_mode.register_fake
def _(x, gravity, aligned, fx, fy, cx, cy, align_corners, mode, rotate):
    return x.new_empty((x.shape[0], 3, 3)), torch.empty_like(x)


@torch.library.custom_op("vidc::warp2dof_fwd_mode_backward", mutates_args=(), device_types=_DEV)
def warp2dof_fwd_mode_backward(dy: torch.Tensor, gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                               align_corners: bool, mode: int, rotate: bool) -> torch.Tensor:
    """dx of warp2dof_fwd_mode: Cg_R_C^T with rotate, then the transposed gather of the mode (vidc_warp2dof_fwd_mode_backward)."""
    wp = _warper(dy, fx, fy, cx, cy, align_corners)
    assert tuple(dy.shape[-2:]) == (wp.H, wp.W)
    return _ops.warp2dof_fwd_mode_backward(dy, wp._params(gravity, aligned), cx, cy, align_corners, mode, rotate)


@warp2dof_fwd_mode_backward.register_fake
def _(dy, gravity, aligned, fx, fy, cx, cy, align_corners, mode, rotate):
    return torch.empty_like(dy)


_register_warp_autograd("warp2dof_fwd_mode", "warp2dof_fwd_mode_backward", 7)


@torch.library.custom_op("vidc::warp2dof_grids", mutates_args=(), device_types=_DEV)
def warp2dof_grids(gravity: torch.Tensor, aligned: torch.Tensor, fx: float, fy: float, cx: float, cy: float, W: int,
                   H: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(C_R_Cg (B,3,3), grid (B,H,W,2), inverse grid (B,H,W,2)) -- Warping2DOFAlignment.image_sampler_forward_inverse; W, H must be the ones the
    intrinsics give (ceil(2 cx), ceil(2 cy)).  Not differentiable (no autograd formula is registered: the geometry gets no gradient)."""
    wp = _warper(gravity, fx, fy, cx, cy, False)
    assert (W, H) == (wp.W, wp.H), "W, H must be ceil(2 cx), ceil(2 cy) = %d, %d" % (wp.W, wp.H)
    return wp.image_sampler_forward_inverse(gravity, aligned)


@warp2dof_grids.register_fake
def _(gravity, aligned, fx, fy, cx, cy, W, H):
    B = gravity.shape[0]
    return gravity.new_empty((B, 3, 3)), gravity.new_empty((B, H, W, 2)), gravity.new_empty((B, H, W, 2))


AFFINE_ILL_COND = 4.0       # kAffineIllCond of csrc/train.hip: a power of two, so the product below is exact in fp32 on either side


def affine_reads_raw(scale, shift):
    """Per channel: does vidc_affine_act_backward, given c_raw, read c from it instead of rebuilding it as (y - shift) / scale?  The kernel
    evaluates the same fp32 expression (affine_act_bwd_kernel); conv2d_bn_act_backward states the rule."""
    scale, shift = scale.float(), shift.float()
    return (scale == 0) | (shift.abs() > AFFINE_ILL_COND * scale.abs())


def _conv_backward_body(what, dy, x_nhwc, w_oihw, y, scale, shift, in_h, in_w, stride, pad, dilation, relu, precision, need_x, need_w, need_affine,
                        recompute_c):
    """conv2d_bn_act_backward and conv2d_dilated_bn_act_backward (documented there)."""
    dil = {} if dilation == 1 else {"dilation": dilation}
    c_raw = None
    if need_affine and (recompute_c or bool(affine_reads_raw(scale, shift).any())):
        if x_nhwc is None:
            raise RuntimeError("%s: dscale of this conv needs the conv's input" % what)
        c_raw = _ops.conv2d_bn_act(x_nhwc, _ops.pack_conv_weight(w_oihw), torch.ones_like(scale), torch.zeros_like(shift), w_oihw.shape[2],
                                   w_oihw.shape[3], stride=stride, pad=pad, precision=0, **dil)
    dc, dscale, dshift = _ops.affine_act_backward(dy, y, scale, shift, relu, c_raw, all_from_raw=recompute_c)
    dx = _ops.conv_backward_data(dc, w_oihw, in_h, in_w, stride, pad, precision, **dil) if need_x else dy.new_empty(0)
    if need_w and x_nhwc is None:
        raise RuntimeError("%s: dw needs the conv's input" % what)
    dw = _ops.conv_backward_weight(dc, x_nhwc, tuple(w_oihw.shape), stride, pad, precision=2 if precision == 2 else 0, **dil) if need_w else dy.new_empty(0)
    return dx, dw, (dscale if need_affine else dy.new_empty(0)), (dshift if need_affine else dy.new_empty(0))


def _conv_backward_shapes(dy, w_oihw, scale, shift, in_h, in_w, need_x, need_w, need_affine):
    """The shape function of both conv backward operators: a gradient that is not needed is empty."""
    empty = lambda: dy.new_empty(0)
    return (dy.new_empty((dy.shape[0], in_h, in_w, w_oihw.shape[1])) if need_x else empty(), torch.empty_like(w_oihw) if need_w else empty(),
            torch.empty_like(scale) if need_affine else empty(), torch.empty_like(shift) if need_affine else empty())


@torch.library.custom_op("vidc::conv2d_bn_act_backward", mutates_args=(), device_types=_DEV)
def conv2d_bn_act_backward(dy: torch.Tensor, x_nhwc: Optional[torch.Tensor], w_oihw: torch.Tensor, y: torch.Tensor, scale: torch.Tensor,
                           shift: torch.Tensor, in_h: int, in_w: int, stride: int, pad: int, relu: bool, precision: int, need_x: bool,
                           need_w: bool, need_affine: bool, recompute_c: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dw, dscale, dshift) of relu?(conv(x, w) * scale + shift); a gradient that is not needed comes back empty.  The epilogue is
    transposed first (vidc_affine_act_backward -> dc, dscale, dshift); dx = the conv kernel on data-gradient weights over dc (zero-stuffed when
    strided) in the arithmetic of `precision`; dw = vidc_conv_wgrad in fp32.  `precision` here is the data gradient's: the forward's for a
    Winograd forward, 0 for the direct form -- tests/test_torch_ops.py holds the direct form at precision 1 to the fp32 tolerance, so its
    gradient is held to fp32 accuracy as well, which split-bf16 products (~2^-16 each) miss by 1.5-6 x (profiles/EXPERIMENTS.md); Winograd
    at precision 1 is granted 10 x fp32 and keeps the faster arithmetic.  dscale sums mask(dy) * c with c = (y - shift) / scale; with
    recompute_c (the forward ran in bf16x3 or as Winograd, whose y is not an fp32-accurate image of c), and for channels whose scale is 0, c
    is read from a re-run of the conv in the direct fp32 form with an identity epilogue, so that dscale is an fp32 result like dw and dshift.
    The same holds for an ill-conditioned channel, |shift| > AFFINE_ILL_COND * |scale| (affine_reads_raw; a folded BatchNorm with a small
    gamma / sigma makes such channels): y = fl(c * scale + shift) is exact to u * max(|c * scale|, |shift|) only, so the quotient gives c to
    u * (|c| + |shift / scale|) -- at most u * (|c| + AFFINE_ILL_COND) where the rule keeps the quotient, which for a conv output of the order
    of 1 is less than the fp32 conv's own rounding of c, and nothing where it does not (scale 1e-30, shift 1: y == shift, c == 0).  The rule
    is evaluated here, on the host, from scale and shift alone (it assumes that order of c); the conv is re-run only if it names a channel,
    and the kernel applies the same fp32 comparison per channel, so the channels it keeps have the bits of a call without the re-run.
    x_nhwc is read by dw and by that re-run.
    precision 2 (recorded inside grad_precision(2)): dx = the conv kernel at plain bf16 on pack kind 5 weights over the bf16 cast of dc, and dw =
    vidc_conv_wgrad_bf16 (dc and x rounded to bf16, fp32 accumulation), each where ops.conv_backward_data_precision /
    ops.conv_backward_weight_precision allow it and in fp32 otherwise; dc, dscale, dshift and the c_raw re-run stay fp32 and untouched."""
    return _conv_backward_body("conv2d_bn_act_backward", dy, x_nhwc, w_oihw, y, scale, shift, in_h, in_w, stride, pad, 1, relu, precision, need_x, need_w,
                               need_affine, recompute_c)


@conv2d_bn_act_backward.register_fake
def _(dy, x_nhwc, w_oihw, y, scale, shift, in_h, in_w, stride, pad, relu, precision, need_x, need_w, need_affine, recompute_c):
    return _conv_backward_shapes(dy, w_oihw, scale, shift, in_h, in_w, need_x, need_w, need_affine)


@torch.library.custom_op("vidc::conv2d_dilated_bn_act_backward", mutates_args=(), device_types=_DEV)
def conv2d_dilated_bn_act_backward(dy: torch.Tensor, x_nhwc: Optional[torch.Tensor], w_oihw: torch.Tensor, y: torch.Tensor, scale: torch.Tensor,
                                   shift: torch.Tensor, in_h: int, in_w: int, pad: int, dilation: int, relu: bool, precision: int, need_x: bool,
                                   need_w: bool, need_affine: bool, recompute_c: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dw, dscale, dshift) of conv2d_dilated_bn_act, as conv2d_bn_act_backward with stride 1: vidc_affine_act_backward -> dc; dx = the conv kernel
    on the data-gradient weights over dc with the same dilation and pad' = dilation * (k - 1) - pad, in the arithmetic of `precision` (the
    registration passes 0: the direct form's data gradient is exact fp32); dw = vidc_conv_wgrad_dilated in fp32; dscale's re-run of the conv
    (recompute_c, or a zero scale) is dilated as well.  precision 2 (grad_precision(2)): dx and dw in plain bf16 as in conv2d_bn_act_backward, dw through
    vidc_conv_wgrad_bf16 with the dilation; dc, dscale, dshift and the re-run stay fp32."""
    return _conv_backward_body("conv2d_dilated_bn_act_backward", dy, x_nhwc, w_oihw, y, scale, shift, in_h, in_w, 1, pad, dilation, relu, precision, need_x,
                               need_w, need_affine, recompute_c)


@conv2d_dilated_bn_act_backward.register_fake
def _(dy, x_nhwc, w_oihw, y, scale, shift, in_h, in_w, pad, dilation, relu, precision, need_x, need_w, need_affine, recompute_c):
    return _conv_backward_shapes(dy, w_oihw, scale, shift, in_h, in_w, need_x, need_w, need_affine)


def _conv_setup_common(ctx, what, x, w, scale, shift, y, geometry, relu, precision, needs, winograd=False):
    """Saves what the backward operator reads and builds ctx.args, its arguments after the six tensors; geometry: its two after in_h, in_w -- (stride, pad), or
    (pad, dilation) for the dilated operator."""
    if precision not in (0, 1):
        raise RuntimeError("torch.ops.vidc.%s: precision %d (plain bf16 is 2, MXFP8 is 3) has no backward; use precision 0 or 1 for inputs that require a gradient"
                           % (what, precision))
    need_x, need_w, need_affine = needs[0], needs[1], needs[2] or needs[3]
    ctx.save_for_backward(x if (need_w or need_affine) else None, w, y, scale, shift)      # (dscale re-runs the conv where a scale is 0)
    dgrad_precision = precision if winograd else 0      # (see conv2d_bn_act_backward)
    if current_grad_precision() == 2:                   # grad_precision(2): both conv gradients in plain bf16, whatever the forward ran in
        dgrad_precision = 2
    ctx.args = (x.shape[1], x.shape[2]) + geometry + (relu, dgrad_precision, need_x, need_w, need_affine, bool(needs[2] and (precision == 1 or winograd)))


def _conv_grads(ctx, grad_y, backward_op, n_other):
    """The autograd tuple of a conv forward with n_other arguments behind x, w, scale, shift, from backward_op's four tensors."""
    x, w, y, scale, shift = ctx.saved_tensors
    dx, dw, dscale, dshift = backward_op(grad_y, x, w, y, scale, shift, *ctx.args)
    return (_none_if_empty(dx), _none_if_empty(dw), dscale.reshape(scale.shape) if ctx.needs_input_grad[2] else None,
            dshift.reshape(shift.shape) if ctx.needs_input_grad[3] else None) + (None,) * n_other


def _conv_setup(ctx, inputs, output):
    x, w, scale, shift, stride, pad, relu, precision = inputs
    _conv_setup_common(ctx, "conv2d_bn_act", x, w, scale, shift, output, (stride, pad), relu, precision, ctx.needs_input_grad)


def _wino_setup(ctx, inputs, output):
    x, w, scale, shift, m, relu, precision = inputs
    # the gradient of a 3x3 conv does not care how the forward was evaluated: the direct form's backward with stride 1 / pad 1
    _conv_setup_common(ctx, "conv3x3_winograd", x, w, scale, shift, output, (1, 1), relu, precision, ctx.needs_input_grad, winograd=True)


def _dilated_setup(ctx, inputs, output):
    x, w, scale, shift, pad, dilation, relu, precision = inputs
    if w.shape[2] != w.shape[3] or dilation < 1 or dilation * (w.shape[2] - 1) - pad < 0:
        raise RuntimeError("torch.ops.vidc.conv2d_dilated_bn_act: the backward covers square kernels with pad <= dilation * (k - 1) (got %dx%d, pad %d, "
                           "dilation %d)" % (w.shape[2], w.shape[3], pad, dilation))
    _conv_setup_common(ctx, "conv2d_dilated_bn_act", x, w, scale, shift, output, (pad, dilation), relu, precision, ctx.needs_input_grad)


torch.library.register_autograd("vidc::conv2d_bn_act", lambda ctx, g: _conv_grads(ctx, g, torch.ops.vidc.conv2d_bn_act_backward, 4), setup_context=_conv_setup)
torch.library.register_autograd("vidc::conv3x3_winograd", lambda ctx, g: _conv_grads(ctx, g, torch.ops.vidc.conv2d_bn_act_backward, 3), setup_context=_wino_setup)
torch.library.register_autograd("vidc::conv2d_dilated_bn_act", lambda ctx, g: _conv_grads(ctx, g, torch.ops.vidc.conv2d_dilated_bn_act_backward, 4),
                                setup_context=_dilated_setup)


@torch.library.custom_op("vidc::stem_conv3x3s2_backward", mutates_args=(), device_types=_DEV)
def stem_conv3x3s2_backward(dy: torch.Tensor, x_nchw: Optional[torch.Tensor], w_oihw: torch.Tensor, y: torch.Tensor, in_h: int, in_w: int,
                            relu: bool, need_x: bool, need_w: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx NCHW, dw) of stem_conv3x3s2: vidc_stem_conv3x3s2_backward_data / vidc_stem_wgrad; a gradient that is not needed comes back empty."""
    dx = _ops.stem_conv3x3s2_backward_data(dy, y, w_oihw, in_h, in_w, relu) if need_x else dy.new_empty(0)
    if need_w and x_nchw is None:
        raise RuntimeError("stem_conv3x3s2_backward: dw needs the conv's input")
    dw = _ops.stem_conv3x3s2_backward_weight(dy, y, x_nchw, tuple(w_oihw.shape), relu) if need_w else dy.new_empty(0)
    return dx, dw


@stem_conv3x3s2_backward.register_fake
def _(dy, x_nchw, w_oihw, y, in_h, in_w, relu, need_x, need_w):
    return (dy.new_empty((dy.shape[0], w_oihw.shape[1], in_h, in_w)) if need_x else dy.new_empty(0),
            torch.empty_like(w_oihw) if need_w else dy.new_empty(0))


def _stem_setup(ctx, inputs, output):
    x, w, relu = inputs
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    ctx.save_for_backward(x if need_w else None, w, output)
    ctx.args = (x.shape[2], x.shape[3], relu, need_x, need_w)


def _stem_backward(ctx, grad_y):
    x, w, y = ctx.saved_tensors
    dx, dw = torch.ops.vidc.stem_conv3x3s2_backward(grad_y, x, w, y, *ctx.args)
    return _none_if_empty(dx), _none_if_empty(dw), None


torch.library.register_autograd("vidc::stem_conv3x3s2", _stem_backward, setup_context=_stem_setup)


@torch.library.custom_op("vidc::maxpool3x3s2_backward", mutates_args=(), device_types=_DEV)
def maxpool3x3s2_backward(dy: torch.Tensor, x_nhwc: torch.Tensor) -> torch.Tensor:
    return _ops.maxpool3x3s2_backward(dy, x_nhwc)


@maxpool3x3s2_backward.register_fake
def _(dy, x_nhwc):
    return torch.empty_like(x_nhwc)


def _maxpool_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _maxpool_backward(ctx, grad_y):
    return torch.ops.vidc.maxpool3x3s2_backward(grad_y, ctx.saved_tensors[0])


torch.library.register_autograd("vidc::maxpool3x3s2", _maxpool_backward, setup_context=_maxpool_setup)


@torch.library.custom_op("vidc::avgpool2d_backward", mutates_args=(), device_types=_DEV)
def avgpool2d_backward(dy: torch.Tensor, in_h: int, in_w: int, kh: int, kw: int, sh: int, sw: int, ph: int, pw: int) -> torch.Tensor:
    """dx NHWC (B, in_h, in_w, C) of avgpool2d (vidc_avgpool2d_backward: a deterministic gather)."""
    return _ops.avgpool2d_backward(dy, (in_h, in_w), (kh, kw), (sh, sw), (ph, pw))


@avgpool2d_backward.register_fake
def _(dy, in_h, in_w, kh, kw, sh, sw, ph, pw):
    return dy.new_empty((dy.shape[0], in_h, in_w, dy.shape[3]))


def _avgpool_setup(ctx, inputs, output):
    x, *geom = inputs
    ctx.args = (x.shape[1], x.shape[2]) + tuple(geom)


def _avgpool_backward(ctx, grad_y):
    return (torch.ops.vidc.avgpool2d_backward(grad_y, *ctx.args),) + (None,) * 6


torch.library.register_autograd("vidc::avgpool2d", _avgpool_backward, setup_context=_avgpool_setup)


@torch.library.custom_op("vidc::upsample_bilinear_ac_backward", mutates_args=(), device_types=_DEV)
def upsample_bilinear_ac_backward(dy: torch.Tensor, y: Optional[torch.Tensor], in_h: int, in_w: int) -> torch.Tensor:
    """dx of upsample_bilinear_ac; y: the forward output when its ReLU was applied (vidc_relu_backward first), else None."""
    return _ops.upsample_bilinear_ac_backward(dy, (in_h, in_w), y)


@upsample_bilinear_ac_backward.register_fake
def _(dy, y, in_h, in_w):
    return dy.new_empty((dy.shape[0], in_h, in_w, dy.shape[3]))


def _upsample_setup(ctx, inputs, output):
    x, _oh, _ow, relu = inputs
    ctx.save_for_backward(output if relu else None)
    ctx.args = (x.shape[1], x.shape[2])


def _upsample_backward(ctx, grad_y):
    return torch.ops.vidc.upsample_bilinear_ac_backward(grad_y, ctx.saved_tensors[0], *ctx.args), None, None, None


torch.library.register_autograd("vidc::upsample_bilinear_ac", _upsample_backward, setup_context=_upsample_setup)


@torch.library.custom_op("vidc::head_conv1x1_upsample_backward", mutates_args=(), device_types=_DEV)
def head_conv1x1_upsample_backward(dy: torch.Tensor, x_nhwc: torch.Tensor, w: torch.Tensor, y: Optional[torch.Tensor],
                                   pad: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx NHWC, dw, dbias (Cout,)) of head_conv1x1_upsample: vidc_relu_backward (y given), vidc_upsample_bilinear_ac_backward on the B * Cout
    one-channel planes, vidc_head_backward_multi.  Up to four output channels, pad 0 or 1."""
    return _ops.head_conv1x1_upsample_backward(dy, x_nhwc, w, pad, y)


@head_conv1x1_upsample_backward.register_fake
def _(dy, x_nhwc, w, y, pad):
    return torch.empty_like(x_nhwc), torch.empty_like(w), dy.new_empty((w.shape[0],))


def _head_setup(ctx, inputs, output):
    x, w, bias, pad, _oh, _ow, relu = inputs
    if not 1 <= w.shape[0] <= 4 or pad not in (0, 1):
        raise RuntimeError("torch.ops.vidc.head_conv1x1_upsample: the backward covers 1 to 4 output channels and pad 0 or 1 only (got Cout %d, pad %d)"
                           % (w.shape[0], pad))
    ctx.save_for_backward(x, w, output if relu else None)
    ctx.pad, ctx.bias_shape = pad, bias.shape


def _head_backward(ctx, grad_y):
    x, w, y = ctx.saved_tensors
    dx, dw, db = torch.ops.vidc.head_conv1x1_upsample_backward(grad_y, x, w, y, ctx.pad)
    need = ctx.needs_input_grad
    return (dx if need[0] else None, dw if need[1] else None, db.reshape(ctx.bias_shape) if need[2] else None, None, None, None, None)


torch.library.register_autograd("vidc::head_conv1x1_upsample", _head_backward, setup_context=_head_setup)


# ---- training SurfaceNormalDORN: train-mode BatchNorm, Dropout2d, F.normalize, the normal loss ---------------------------------------------
# batch_norm_train writes the running statistics in place, and torch.library.custom_op registers no autograd formula for an operator that mutates
# an argument: it is defined through torch.library.define / impl -- the schema declares the two mutated arguments (what mutates_args would), the kernel
# is registered for the GPU dispatch key only, and the Autograd key runs _BatchNormTrain, whose backward is the custom_op batch_norm_train_backward.
torch.library.define("vidc::batch_norm_train", "(Tensor x_nhwc, Tensor gamma, Tensor beta, Tensor(a!) running_mean, Tensor(b!) running_var, float momentum, "
                     "float eps, bool relu, Tensor? residual=None) -> (Tensor, Tensor, Tensor)")


@torch.library.impl("vidc::batch_norm_train", "CUDA")
def batch_norm_train(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    """(y, save_mean, save_rstd): y = relu?(nn.BatchNorm2d in train() mode (x) + residual) on NHWC; the batch statistics over the B*H*W rows in fp64,
    save_mean / save_rstd (C,) kept for the backward; running_mean / running_var updated in place as nn.BatchNorm2d updates them (momentum, unbiased
    variance).  x and residual may be channel slices of wider tensors.  vidc_bn_train_forward_add: the kernels of the trainers' BatchNorm."""
    return _ops.batch_norm_train(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual)


@torch.library.register_fake("vidc::batch_norm_train")
def _(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    Cc = x_nhwc.shape[-1]
    return x_nhwc.new_empty(x_nhwc.shape), x_nhwc.new_empty((Cc,)), x_nhwc.new_empty((Cc,))


@torch.library.custom_op("vidc::batch_norm_train_backward", mutates_args=(), device_types=_DEV)
def batch_norm_train_backward(dy: torch.Tensor, x_nhwc: torch.Tensor, y: Optional[torch.Tensor], gamma: torch.Tensor, save_mean: torch.Tensor,
                              save_rstd: torch.Tensor, has_residual: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma, dbeta, dresidual) of batch_norm_train; y: the forward output when its ReLU was applied, else None.  vidc_bn_train_backward, and
    with a residual vidc_relu_backward first: the masked gradient is dresidual and what the BatchNorm part starts from (no residual: empty)."""
    return _ops.batch_norm_train_backward(dy, x_nhwc, y, gamma, save_mean, save_rstd, has_residual)


@batch_norm_train_backward.register_fake
def _(dy, x_nhwc, y, gamma, save_mean, save_rstd, has_residual):
    Cc = x_nhwc.shape[-1]
    return (x_nhwc.new_empty(x_nhwc.shape), x_nhwc.new_empty((Cc,)), x_nhwc.new_empty((Cc,)),
            x_nhwc.new_empty(x_nhwc.shape) if has_residual else x_nhwc.new_empty(0))


class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual):
        with torch._C._AutoDispatchBelowAutograd():
            y, mean, rstd = torch.ops.vidc.batch_norm_train(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual)
        ctx.save_for_backward(x, y if relu else None, gamma, mean, rstd)
        ctx.has_residual = residual is not None
        ctx.mark_non_differentiable(mean, rstd)
        ctx.set_materialize_grads(False)
        return y, mean, rstd

    @staticmethod
    def backward(ctx, grad_y, _grad_mean, _grad_rstd):
        x, y, gamma, mean, rstd = ctx.saved_tensors
        if grad_y is None:
            return (None,) * 9
        dx, dgamma, dbeta, dres = torch.ops.vidc.batch_norm_train_backward(grad_y, x, y, gamma, mean, rstd, ctx.has_residual)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dgamma.reshape(gamma.shape) if need[1] else None, dbeta.reshape(gamma.shape) if need[2] else None, None, None, None,
                None, None, dres if (ctx.has_residual and need[8]) else None)


@torch.library.impl("vidc::batch_norm_train", "Autograd")
def _batch_norm_train_autograd(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    return _BatchNormTrain.apply(x_nhwc, gamma, beta, running_mean, running_var, momentum, eps, relu, residual)


# batch_norm_eval is the frozen form (nn.BatchNorm2d in eval() mode inside a training step): it reads the running statistics and mutates nothing, so it
# is a plain custom_op with a registered autograd formula.  The backward computes only what somebody needs: without a gradient for gamma / beta it is one
# elementwise launch that reads neither x (which is then not even saved) nor any scratch; without one for x no dx is written.
@torch.library.custom_op("vidc::batch_norm_eval", mutates_args=(), device_types=_DEV)
def batch_norm_eval(x_nhwc: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor, eps: float,
                    relu: bool, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = relu?(nn.BatchNorm2d in eval() mode (x) + residual) on NHWC: (x - running_mean) / sqrt(running_var + eps) * gamma + beta, the running
    statistics read and left alone.  x and residual may be channel slices of wider tensors.  vidc_bn_eval_forward_add, one launch."""
    return _ops.batch_norm_eval(x_nhwc, gamma, beta, running_mean, running_var, eps, relu, residual)


@batch_norm_eval.register_fake
def _(x_nhwc, gamma, beta, running_mean, running_var, eps, relu, residual=None):
    return x_nhwc.new_empty(x_nhwc.shape)


@torch.library.custom_op("vidc::batch_norm_eval_backward", mutates_args=(), device_types=_DEV)
def batch_norm_eval_backward(dy: torch.Tensor, x_nhwc: Optional[torch.Tensor], y: Optional[torch.Tensor], gamma: torch.Tensor, running_mean: torch.Tensor,
                             running_var: torch.Tensor, eps: float, has_residual: bool, need_dx: bool,
                             need_affine: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma, dbeta, dresidual) of batch_norm_eval, each empty when not computed: dx unless need_dx, dgamma / dbeta unless need_affine (x is read
    for them only and may be None otherwise), dresidual unless a residual sits in front of a ReLU (y given: the masked gradient, which the BatchNorm part
    starts from; without a ReLU the masked gradient is dy itself).  vidc_bn_eval_backward."""
    return _ops.batch_norm_eval_backward(dy, x_nhwc, y, gamma, running_mean, running_var, eps, has_residual, need_dx, need_affine)


@batch_norm_eval_backward.register_fake
def _(dy, x_nhwc, y, gamma, running_mean, running_var, eps, has_residual, need_dx, need_affine):
    Cc = dy.shape[-1]
    return (dy.new_empty(dy.shape if need_dx else (0,)), dy.new_empty((Cc if need_affine else 0,)), dy.new_empty((Cc if need_affine else 0,)),
            dy.new_empty(dy.shape if (has_residual and y is not None) else (0,)))


def _bn_eval_setup(ctx, inputs, output):
    x, gamma, beta, running_mean, running_var, eps, relu, residual = inputs
    need = ctx.needs_input_grad
    ctx.need_affine = bool(need[1] or need[2])
    ctx.save_for_backward(x if ctx.need_affine else None, output if relu else None, gamma, running_mean, running_var)
    ctx.eps, ctx.has_residual, ctx.param_shape = eps, residual is not None, gamma.shape


def _bn_eval_backward(ctx, grad_y):
    x, y, gamma, running_mean, running_var = ctx.saved_tensors
    need = ctx.needs_input_grad
    has_res = ctx.has_residual and need[7]
    dx, dgamma, dbeta, dres = torch.ops.vidc.batch_norm_eval_backward(grad_y, x, y, gamma, running_mean, running_var, ctx.eps, has_res, need[0], ctx.need_affine)
    if has_res and y is None:
        dres = grad_y                                # no ReLU behind the sum: the residual's gradient is the incoming one itself
    return (dx if need[0] else None, dgamma.reshape(ctx.param_shape) if need[1] else None, dbeta.reshape(ctx.param_shape) if need[2] else None, None, None,
            None, None, dres if has_res else None)


torch.library.register_autograd("vidc::batch_norm_eval", _bn_eval_backward, setup_context=_bn_eval_setup)


@torch.library.custom_op("vidc::scale_image_channels", mutates_args=(), device_types=_DEV)
def scale_image_channels(x_nhwc: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """y[b,h,w,c] = x[b,h,w,c] * keep[b][c] (vidc_scale_image_channels): Dropout2d's forward for a given keep table, and its own backward."""
    return _ops.scale_image_channels(x_nhwc, keep)


@scale_image_channels.register_fake
def _(x_nhwc, keep):
    return x_nhwc.new_empty(x_nhwc.shape)


def _scale_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _scale_backward(ctx, grad_y):
    return torch.ops.vidc.scale_image_channels(grad_y, ctx.saved_tensors[0]), None      # (keep gets no gradient)


torch.library.register_autograd("vidc::scale_image_channels", _scale_backward, setup_context=_scale_setup)


@torch.library.custom_op("vidc::dropout2d", mutates_args=(), device_types=_DEV)
def dropout2d(x_nhwc: torch.Tensor, p: float, seed: int, offset: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """nn.Dropout2d(p) in train() mode on NHWC: (y, keep) with keep (B, C) = 0 or 1 / (1 - p), one Philox4x32-10 draw per (image, channel) at
    (seed, offset) (vidc_dropout2d_mask; torch's own random stream is not reproduced), y = x * keep (vidc_scale_image_channels)."""
    keep = _ops.dropout2d_mask(x_nhwc.shape[0], x_nhwc.shape[-1], p, seed, offset, x_nhwc.device)
    return _ops.scale_image_channels(x_nhwc, keep), keep


@dropout2d.register_fake
def _(x_nhwc, p, seed, offset):
    return x_nhwc.new_empty(x_nhwc.shape), x_nhwc.new_empty((x_nhwc.shape[0], x_nhwc.shape[-1]))


def _dropout_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _dropout_backward(ctx, grad_y, _grad_keep):
    return (torch.ops.vidc.scale_image_channels(grad_y, ctx.saved_tensors[0]) if grad_y is not None else None), None, None, None


torch.library.register_autograd("vidc::dropout2d", _dropout_backward, setup_context=_dropout_setup)


@torch.library.custom_op("vidc::normalize_nchw", mutates_args=(), device_types=_DEV)
def normalize_nchw(x: torch.Tensor) -> torch.Tensor:
    """F.normalize(x, dim=1) on NCHW (vidc_normalize_nchw; surface_normal_dorn.py:154)."""
    return _ops.normalize_nchw(x)


@normalize_nchw.register_fake
def _(x):
    return x.new_empty(x.shape)


@torch.library.custom_op("vidc::normalize_nchw_backward", mutates_args=(), device_types=_DEV)
def normalize_nchw_backward(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dx of normalize_nchw (vidc_normalize_nchw_backward): (dy - n (n . dy)) / |x|, and dy / eps where |x| < eps = 1e-12, as torch's."""
    return _ops.normalize_nchw_backward(x, dy)


@normalize_nchw_backward.register_fake
def _(x, dy):
    return x.new_empty(x.shape)


def _normalize_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _normalize_backward(ctx, grad_y):
    return torch.ops.vidc.normalize_nchw_backward(ctx.saved_tensors[0], grad_y)


torch.library.register_autograd("vidc::normalize_nchw", _normalize_backward, setup_context=_normalize_setup)


def _scale_dpred(dpred: torch.Tensor, grad_loss: torch.Tensor) -> torch.Tensor:
    """dpred * grad_loss (a one-element tensor read on the device: no host read), through vidc_scale_image_channels."""
    return _ops.scale_by_scalar(dpred, grad_loss)


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[3])
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _register_l1_loss_backward(name, n_inputs):
    """What normal_l1_loss and depth_l1_loss share behind vidc::`name`_with_grad -> (loss, two statistics, dpred): the operator vidc::`name`_backward
    (_scale_dpred), and the autograd formula that hands it the saved dpred and the loss's gradient; only pred, the first of the n_inputs, gets a gradient."""
    op = torch.library.custom_op("vidc::%s_backward" % name, _scale_dpred, mutates_args=(), device_types=_DEV)
    op.register_fake(lambda dpred, grad_loss: dpred.new_empty(dpred.shape))
    packet = getattr(torch.ops.vidc, "%s_backward" % name)

    def backward(ctx, grad_loss, _g1, _g2, _gd):
        if grad_loss is None:
            return (None,) * n_inputs
        return (packet(ctx.saved_tensors[0], grad_loss),) + (None,) * (n_inputs - 1)

    torch.library.register_autograd("vidc::%s_with_grad" % name, backward, setup_context=_loss_setup)
    return op


@torch.library.custom_op("vidc::normal_l1_loss_with_grad", mutates_args=(), device_types=_DEV)
def normal_l1_loss_with_grad(pred: torch.Tensor, normal_gt: torch.Tensor, mask: torch.Tensor,
                             normalize_prediction: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss, count, angle, dpred): normal_l1_loss with the gradient the same vidc_normal_l1_loss call wrote -- what normal_l1_loss saves for its backward."""
    sums, dpred = _ops.normal_l1_loss(pred, normal_gt, mask, normalize_prediction)
    s32 = sums.float()                       # the kernel's fp64 sums, rounded once
    return s32[0:1].clone(), s32[1:2].clone(), s32[2:3].clone(), dpred


@normal_l1_loss_with_grad.register_fake
def _(pred, normal_gt, mask, normalize_prediction):
    return pred.new_empty((1,)), pred.new_empty((1,)), pred.new_empty((1,)), pred.new_empty(pred.shape)


normal_l1_loss_backward = _register_l1_loss_backward("normal_l1_loss", 4)      # (normal_gt and mask get no gradient)

# normal_l1_loss(pred, normal_gt, mask, normalize_prediction) -> (loss, count, angle): the first three outputs of normal_l1_loss_with_grad.  Registered for
# every backend as that composition, so its shape function, its GPU-only dispatch and its autograd formula are that operator's.
torch.library.define("vidc::normal_l1_loss", "(Tensor pred, Tensor normal_gt, Tensor mask, bool normalize_prediction) -> (Tensor, Tensor, Tensor)")


@torch.library.impl("vidc::normal_l1_loss", "CompositeImplicitAutograd")
def normal_l1_loss(pred, normal_gt, mask, normalize_prediction):
    """(loss, count, angle), float32 tensors of one element rounded from vidc_normal_l1_loss's fp64 sums (network_run.py:181-189): loss = the masked L1
    distance to F.normalize(normal_gt) per masked pixel, differentiable in pred (backward: dpred * grad_loss, dpred written by the forward's one kernel
    call); count = the masked pixels, angle = the summed angular error in degrees: not differentiable."""
    loss, count, angle, _dpred = torch.ops.vidc.normal_l1_loss_with_grad(pred, normal_gt, mask, normalize_prediction)
    return loss, count, angle



# ---- training ModifiedFPN and SurfaceNormalPrediction under autograd: the depth loss, the use_mask multiply, the decoder's sum -----------------------
@torch.library.custom_op("vidc::depth_l1_loss_with_grad", mutates_args=(), device_types=_DEV)
def depth_l1_loss_with_grad(pred: torch.Tensor, depth_gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss, count, ratios, dpred): depth_l1_loss with the gradient the same vidc_depth_l1_loss call wrote -- what depth_l1_loss saves for its backward."""
    sums, dpred = _ops.depth_l1_loss(pred, depth_gt)
    s32 = sums.float()                       # the kernel's fp64 sums, rounded once (the counts are integers below 2^24 for any batch of 240 x 320 images)
    return s32[0:1].clone(), s32[1:2].clone(), s32[2:7].clone(), dpred


@depth_l1_loss_with_grad.register_fake
def _(pred, depth_gt):
    return pred.new_empty((1,)), pred.new_empty((1,)), pred.new_empty((5,)), pred.new_empty(pred.shape)


depth_l1_loss_backward = _register_l1_loss_backward("depth_l1_loss", 2)      # (depth_gt gets no gradient)

# depth_l1_loss(pred, depth_gt) -> (loss, count, ratios): the first three outputs of depth_l1_loss_with_grad, registered as that composition like normal_l1_loss.
torch.library.define("vidc::depth_l1_loss", "(Tensor pred, Tensor depth_gt) -> (Tensor, Tensor, Tensor)")


@torch.library.impl("vidc::depth_l1_loss", "CompositeImplicitAutograd")
def depth_l1_loss(pred, depth_gt):
    """(loss (1,), count (1,), ratios (5,)), float32 tensors rounded from vidc_depth_l1_loss's fp64 sums: the depth half of `_network_loss`
    (network_run.py:165-179) on pred, depth_gt (B,1,H,W).  loss = the L1 distance summed over depth_gt > 0, divided by H * W: differentiable in pred
    (backward: dpred * grad_loss, dpred written by the forward's one kernel call).  count = the valid pixels, ratios = those of them with
    max(pred / gt, gt / pred) below 1.05, 1.10, 1.25, 1.25^2, 1.25^3: not differentiable; depth_printable_ratios turns them into the reference's dictionary."""
    loss, count, ratios, _dpred = torch.ops.vidc.depth_l1_loss_with_grad(pred, depth_gt)
    return loss, count, ratios


def depth_printable_ratios(count, ratios):
    """GetDepthPrintableRatios (network_run.py:72-82) from depth_l1_loss's count and ratios (tensors or numbers; tensors are read to the host here):
    {'D_1.05': round(100 * c / (n + 1e-7), 1), ...}."""
    n = float(count.reshape(-1)[0]) if torch.is_tensor(count) else float(count)
    cs = ratios.reshape(-1).tolist() if torch.is_tensor(ratios) else list(ratios)
    if len(cs) != len(RATIO_KEYS):
        raise ValueError("depth_printable_ratios: %d counts for %d thresholds" % (len(cs), len(RATIO_KEYS)))
    return {k: round(100 * float(c) / (n + 1e-7), 1) for k, c in zip(RATIO_KEYS, cs)}


@torch.library.custom_op("vidc::feature_mask_scale", mutates_args=(), device_types=_DEV)
def feature_mask_scale(x_nhwc: torch.Tensor, image_nchw: torch.Tensor) -> torch.Tensor:
    """x * F.interpolate((r + g + b > 1e-2) of image, (h, w), mode="nearest") on NHWC x (B,h,w,C) -- the use_mask multiply of surface_normal.py:151-162
    (vidc_mask_scale; the mask is never stored).  x may be a channel slice.  Its own backward on dy; the reference detaches the mask: image gets no gradient."""
    return _ops.feature_mask_scale(x_nhwc, image_nchw)


@feature_mask_scale.register_fake
def _(x_nhwc, image_nchw):
    return x_nhwc.new_empty(x_nhwc.shape)


def _mask_scale_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _mask_scale_backward(ctx, grad_y):
    return torch.ops.vidc.feature_mask_scale(grad_y, ctx.saved_tensors[0]), None


torch.library.register_autograd("vidc::feature_mask_scale", _mask_scale_backward, setup_context=_mask_scale_setup)


@torch.library.custom_op("vidc::add_rows", mutates_args=(), device_types=_DEV)
def add_rows(a: torch.Tensor, b: torch.Tensor, relu: bool) -> torch.Tensor:
    """relu?(a + b) on NHWC tensors of one shape (vidc_add_rows): z1 + z2 + z3 + z4 of both decoders.  a and b may be channel slices."""
    return _ops.add_rows(a, b, relu)


@add_rows.register_fake
def _(a, b, relu):
    return a.new_empty(a.shape)


@torch.library.custom_op("vidc::add_rows_backward", mutates_args=(), device_types=_DEV)
def add_rows_backward(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dy * (y > 0) (vidc_relu_backward): the gradient of both summands of add_rows(a, b, relu=True), y its output."""
    return _ops.relu_backward_rows(dy, y)


@add_rows_backward.register_fake
def _(dy, y):
    return dy.new_empty(dy.shape)


def _add_rows_setup(ctx, inputs, output):
    ctx.save_for_backward(output if inputs[2] else None)


def _add_rows_backward(ctx, grad_y):
    y = ctx.saved_tensors[0]
    g = grad_y if y is None else torch.ops.vidc.add_rows_backward(grad_y, y)      # (without a ReLU the sum hands grad_y itself to both summands)
    return (g if ctx.needs_input_grad[0] else None), (g if ctx.needs_input_grad[1] else None), None


torch.library.register_autograd("vidc::add_rows", _add_rows_backward, setup_context=_add_rows_setup)


# ---- the operator names, by the layer that added them (tests and INTEGRATION.md pin every tuple) -------------------------------------------------
# the backward operators of the warps, the convs and the glue
BACKWARD_OPS = ("warp2dof_fwd_backward", "warp2dof_inv_rot_norm_backward", "conv2d_bn_act_backward", "stem_conv3x3s2_backward", "maxpool3x3s2_backward",
                "upsample_bilinear_ac_backward", "head_conv1x1_upsample_backward")
# the scene-understanding module of SurfaceNormalDORN
DORN_OPS = ("conv2d_dilated_bn_act", "avgpool2d")
DORN_BACKWARD_OPS = ("conv2d_dilated_bn_act_backward", "avgpool2d_backward")
# SurfaceNormalDORN.forward_autograd and its loss; scale_image_channels is its own backward and dropout2d's
TRAIN_OPS = ("batch_norm_train", "dropout2d", "scale_image_channels", "normalize_nchw", "normal_l1_loss", "normal_l1_loss_with_grad")
TRAIN_BACKWARD_OPS = ("batch_norm_train_backward", "normalize_nchw_backward", "normal_l1_loss_backward")
# ModifiedFPN.forward_autograd, SurfaceNormalPrediction.forward_autograd and the depth loss; feature_mask_scale is its own backward
NET_TRAIN_OPS = ("depth_l1_loss", "depth_l1_loss_with_grad", "feature_mask_scale", "add_rows")
NET_TRAIN_BACKWARD_OPS = ("depth_l1_loss_backward", "add_rows_backward")
# the forward warp in grid_sample's three interpolation modes with its backward, and the sampler grids (not differentiable)
WARP_MODE_OPS = ("warp2dof_fwd_mode", "warp2dof_fwd_mode_backward", "warp2dof_grids")
# a BatchNorm2d in eval() mode under forward_autograd (fine-tuning with frozen BatchNorm) and its backward
FROZEN_BN_OPS = ("batch_norm_eval",)
FROZEN_BN_BACKWARD_OPS = ("batch_norm_eval_backward",)
OPS = (("plane_ransac_normal", "plane_offset", "plane_project_depth", "plane_finalize", "enrich_scatter", "warp2dof_fwd", "warp2dof_inv_rot_norm", "conv2d_bn_act",
        "conv3x3_winograd", "stem_conv3x3s2", "maxpool3x3s2", "upsample_bilinear_ac", "head_conv1x1_upsample")
       + BACKWARD_OPS + DORN_OPS + DORN_BACKWARD_OPS + TRAIN_OPS + TRAIN_BACKWARD_OPS + NET_TRAIN_OPS + NET_TRAIN_BACKWARD_OPS + WARP_MODE_OPS
       + FROZEN_BN_OPS + FROZEN_BN_BACKWARD_OPS)
RATIO_KEYS = ("D_1.05", "D_1.10", "D_1.25", "D_1.56", "D_1.95")      # depth_l1_loss's five ratio counts, as depth_printable_ratios names them
