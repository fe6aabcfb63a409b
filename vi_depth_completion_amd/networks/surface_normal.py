"""Drop-in for the reference's `SurfaceNormalPrediction` (networks/surface_normal.py:57-171): same constructor,
`forward(x, gravity_tensor, alignment_tensor)` and the same 759 state_dict keys, executed as one HIP program:
warp -> ResNet-101 pyramid -> 4-branch decoder -> head -> inverse warp + R^T + L2-normalise.

Training: `SurfaceNormalTrainer` (training.py) is the fast captured step; `forward_autograd(x, gravity, aligned)` is the reference's forward in train()
mode composed of differentiable `torch.ops.vidc` operators on the module's own parameters (use_mask included), for the reference's own loop and any
torch.optim optimizer; `eval()` afterwards re-folds the updated weights for the inference program.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import engine
from .backbone import ResNetPyramids
from . import autograd_blocks
from .fpn_decoder import build_branch, emit_decoder
from .warping_2dof_alignment import Warping2DOFAlignment


class _HipModule(nn.Module):
    """Shared plumbing: derived-weight cache invalidation and per-batch-size program cache."""

    _train_hint = ""           # appended to the train-mode refusal of forward(): where the module's training step lives, if it has one
    _autograd_dirty = False    # a forward_autograd ran since the inference weights were folded (the optimizer steps the parameters behind the module's back)

    def _init_engine(self):
        self._weights = engine.WeightStore(self)
        self._programs = {}
        self._version = 0          # bumped whenever the parameters may have changed (programs spanning modules key on it)
        self.register_load_state_dict_post_hook(lambda m, keys: m._invalidate())

    def _invalidate(self):
        self._weights.invalidate()
        self._programs.clear()
        self._version += 1

    def train(self, mode=True):
        super().train(mode)
        if not mode and self._autograd_dirty:      # eval() after training steps under autograd: the folded weights and the programs are stale
            self._invalidate()
            self._autograd_dirty = False
        return self

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if hasattr(self, "_weights"):
            self._invalidate()
        return r

    def _replicate_for_data_parallel(self):
        # torch.nn.DataParallel (network_run.py:97-99) copies a module per GPU and re-broadcasts its parameters on every forward; a
        # replica of this module would share the packed weights and captured graphs of GPU 0.  Refused, not emulated: frames shard one
        # process per GPU (vi_depth_completion_amd/sharding.py, bench.py --gpus N).
        raise RuntimeError("%s: torch.nn.DataParallel is not supported by the HIP path; run one process per GPU "
                           "(vi_depth_completion_amd.sharding, bench.py --gpus N)" % type(self).__name__)

    def _check(self, *tensors):
        if self.training:
            raise RuntimeError("%s: the HIP path is inference-only (BatchNorm is folded); call .eval()%s" % (type(self).__name__, self._train_hint))
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("%s runs on the GPU only: there is no CPU/eager fallback" % type(self).__name__)

    @staticmethod
    def _execute(prog):
        mode = os.environ.get("VIDC_EXEC", "graph")
        if mode == "graph":
            if not prog.captured:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    prog.run()            # warm-up outside capture (sets kernel attributes)
                    prog.capture()
                torch.cuda.current_stream().wait_stream(side)
            prog.launch()
        else:
            prog.run()


class SurfaceNormalPrediction(_HipModule):
    _train_hint = (", or train the network with vi_depth_completion_amd.training.SurfaceNormalTrainer, or under autograd with "
                   "SurfaceNormalPrediction.forward_autograd (torch.ops.vidc operators)")

    def __init__(self, output_size=(240, 320), in_channels=3, training_mode="train_L2_loss",
                 fc_img=np.array([0.5 * 577.87061, 0.5 * 580.25851]),
                 cc_img=np.array([0.5 * 319.87654, 0.5 * 239.87603]), use_mask=False, align_corners=False):
        super().__init__()
        self.output_size, self.mode, self.use_mask = output_size, training_mode, use_mask
        self.warp_2dof_alignment = Warping2DOFAlignment(fx=fc_img[0], fy=fc_img[1], cx=cc_img[0], cy=cc_img[1],
                                                        align_corners=align_corners)
        self.resnet_pyramids = ResNetPyramids(in_channels=in_channels)
        for lvl in (1, 2, 3, 4):
            setattr(self, "feature%d_upsamping" % lvl, build_branch(lvl, 1))
        self.feature_concat = nn.Sequential(nn.Conv2d(128, 64, 3, 1, 1), nn.ReLU(inplace=True), nn.Conv2d(64, 3, 1),
                                            nn.UpsamplingBilinear2d(size=output_size))
        self._init_engine()

    def build_program(self, B, device, dry_run=False):
        wp = self.warp_2dof_alignment
        prog = engine.Program(self._weights, device, B)
        x = prog.input_nchw("image", self.resnet_pyramids.channel, wp.H, wp.W)
        g = prog.input_raw("gravity", B * 3)
        a = prog.input_raw("aligned", B * 3)
        kinv = prog.input_raw("kinv", 9)
        params = prog.warp_params(g, a, wp, kinv)
        xw = prog.warp_fwd(x, params, wp, wp.align_corners)
        levels = self.resnet_pyramids.emit(prog, xw, engine.K("resnet_pyramids."))
        if self.use_mask:               # surface_normal.py:150-162: features and their sum are zeroed where the warp left no image
            zsum = prog.mask_scale(emit_decoder(prog, self, [prog.mask_scale(t, xw) for t in levels]), xw)
        else:
            zsum = emit_decoder(prog, self, levels)
        h = prog.conv(zsum, "feature_concat.0", relu=True, padding=1)
        y, low = prog.head(h, "feature_concat.2", 0, (wp.H, wp.W), relu=False)
        z = prog.warp_inv(y, params, wp, wp.align_corners, normalize=True)
        prog.mark_output("normals", z)
        prog.mark_output("warped", xw)
        prog.mark_output("warp_params", params)
        prog.taps = {"x%d" % (i + 1): t for i, t in enumerate(levels)}
        prog.taps.update(zsum=zsum, normal_raw=y)
        prog.finalize(dry_run)
        prog.storage[kinv.buf][:9].copy_(wp.kinv(device))
        return prog

    def program(self, B, device, slot=0):
        """Programs are cached per batch size and per `slot` (independent activation buffers sharing the weights), so
        several frames can be in flight on different HIP streams."""
        key = (B, str(device), self.warp_2dof_alignment.align_corners, slot)
        if key not in self._programs:
            self._programs[key] = self.build_program(B, device)
        return self._programs[key]

    def enqueue(self, x, gravity_tensor, alignment_tensor, slot=0):
        """Enqueues one forward pass on the current stream; returns a VIEW of the program's output buffer (valid
        until the next enqueue on the same slot)."""
        self._check(x, gravity_tensor, alignment_tensor)
        B = x.shape[0]
        prog = self.program(B, x.device, slot)
        prog.tensor(prog.inputs["image"]).copy_(x, non_blocking=True)
        prog.storage[prog.inputs["gravity"].buf][: B * 3].copy_(gravity_tensor.reshape(-1), non_blocking=True)
        prog.storage[prog.inputs["aligned"].buf][: B * 3].copy_(alignment_tensor.reshape(-1), non_blocking=True)
        self._execute(prog)
        return prog.tensor(prog.outputs["normals"])

    def forward(self, x, gravity_tensor, alignment_tensor):
        return self.enqueue(x, gravity_tensor, alignment_tensor).clone()

    # ---- training under autograd ---------------------------------------------------------------------------------------------------------
    def forward_autograd(self, x, gravity_tensor, alignment_tensor, precision=0, grad_precision=0):
        """The reference's forward in train() mode (surface_normal.py:147-171) from torch.ops.vidc operators only: warp2dof_fwd, the pyramid and the four
        decoder branches of networks/autograd_blocks.py (train-mode BatchNorm: running statistics and num_batches_tracked updated as torch does; a BatchNorm2d module
        that is itself in eval() mode is frozen: its running statistics are used and left alone), with
        use_mask feature_mask_scale on the four levels and on their sum (the mask is detached, as there), add_rows, feature_concat.0 with its ReLU, the
        three-channel head, warp2dof_inv_rot_norm(normalize=True).  Returns unit normals (B, 3, H, W) with a grad_fn; the gradient reaches x when it
        requires one.  gravity / aligned get no gradient.  precision: the convs' (0 exact fp32, 1 bf16x3).  grad_precision: the arithmetic of
        the convs' data and weight gradients, 0 fp32 (today's backward) or 2 plain bf16 (torch_ops.grad_precision); the stem and the head stay fp32."""
        wp = self.warp_2dof_alignment
        if tuple(x.shape[1:]) != (self.resnet_pyramids.channel, wp.H, wp.W):
            raise ValueError("%s was built for %s inputs, got %s" % (type(self).__name__, (self.resnet_pyramids.channel, wp.H, wp.W), tuple(x.shape[1:])))
        walk = autograd_blocks.begin(self, (x, gravity_tensor, alignment_tensor), precision, grad_precision)
        V = walk.V
        geom = (wp.fx, wp.fy, wp.cx, wp.cy, wp.align_corners)
        xw = V.warp2dof_fwd(x, gravity_tensor, alignment_tensor, *geom)[1]
        levels = walk.pyramid(xw, self.resnet_pyramids)
        if self.use_mask:
            image = xw.detach()
            levels = [V.feature_mask_scale(t, image) for t in levels]
        z = walk.decoder(self, levels)
        if self.use_mask:
            z = V.feature_mask_scale(z, image)
        h = walk.conv(z, self.feature_concat[0], relu=True)
        y = V.head_conv1x1_upsample(h, self.feature_concat[2].weight, self.feature_concat[2].bias, 0, wp.H, wp.W, False)
        walk.finish()
        return V.warp2dof_inv_rot_norm(y, gravity_tensor, alignment_tensor, *geom, True)[1]
