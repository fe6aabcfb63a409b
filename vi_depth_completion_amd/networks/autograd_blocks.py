"""The train() mode forward of the ResNet-101 pyramid and of the four-branch decoder from differentiable `torch.ops.vidc` operators, shared by the
`forward_autograd` of `SurfaceNormalPrediction`, `ModifiedFPN` and `SurfaceNormalDORN` (the reference's networks/surface_normal.py:10-55, 73-145,
networks/depth_completion.py:16-65, 75-147 and networks/surface_normal_dorn.py:79-89, 130-141 as `cnn.train()` runs them).

Every conv is a conv2d_bn_act (dilated: conv2d_dilated_bn_act) with scale 1 and the conv's bias (or 0) as shift; every BatchNorm2d a batch_norm_train on
the batch statistics that updates the module's running statistics in place; the Bottleneck tail is batch_norm_train(residual=identity, relu=True);
z1 + z2 + z3 + z4 is add_rows.
A BatchNorm2d that is itself in eval() mode while the network is in train() mode (the usual way to fine-tune a checkpoint with frozen BatchNorm:
`net.train()`, then `m.eval()` on the BatchNorm modules to freeze, any subset of them) is a batch_norm_eval with the same relu / residual arguments:
it normalises with the running statistics and leaves them and num_batches_tracked alone, as the torch module does.
Unlike the inference program (fpn_decoder.emit_branch) nothing is reordered: a train-mode BatchNorm does not commute with the upsample in front of it.
Activations are NHWC; the module's own parameters and buffers are read, so any torch.optim optimizer steps them.
"""
import torch
import torch.nn as nn


class Walk:
    """One forward pass: the constants the convs share, and the num_batches_tracked counters its BatchNorms touched (`finish` bumps them in one
    launch, as nn.BatchNorm2d does one by one)."""

    def __init__(self, who, device, precision, grad_precision=0):
        if precision not in (0, 1):
            raise RuntimeError("%s.forward_autograd: precision 0 (exact fp32) or 1 (bf16x3); the other conv modes have no backward" % who)
        if grad_precision not in (0, 2):
            raise RuntimeError("%s.forward_autograd: grad_precision 0 (fp32 conv gradients) or 2 (plain bf16 conv gradients)" % who)
        self.who, self.device, self.precision, self.grad_precision = who, device, precision, grad_precision
        self.V = torch.ops.vidc
        self._consts, self._counters = {}, []

    def grads(self):
        """The context every conv of the walk runs its forward in: it records the walk's gradient arithmetic for the conv's backward."""
        from .. import torch_ops                   # (here: torch_ops imports this package)
        return torch_ops.grad_precision(self.grad_precision)

    def const(self, n, v):
        if (n, v) not in self._consts:
            self._consts[(n, v)] = torch.full((n,), v, dtype=torch.float32, device=self.device)
        return self._consts[(n, v)]

    def conv(self, t, m, relu=False):
        co = m.out_channels
        shift = m.bias if m.bias is not None else self.const(co, 0.0)
        with self.grads():
            if m.dilation[0] > 1:
                return self.V.conv2d_dilated_bn_act(t, m.weight, self.const(co, 1.0), shift, m.padding[0], m.dilation[0], relu, self.precision)
            return self.V.conv2d_bn_act(t, m.weight, self.const(co, 1.0), shift, m.stride[0], m.padding[0], relu, self.precision)

    def linear(self, t, m, relu=False):
        """nn.Linear on t (B, h, w, c) flattened as NCHW, run as a 1x1 conv: the weight's (c, h, w) columns reordered to (h, w, c), as engine.linear."""
        B, h, w, c = t.shape
        wt = m.weight.view(-1, c, h, w).permute(0, 2, 3, 1).reshape(-1, h * w * c, 1, 1)
        shift = m.bias if m.bias is not None else self.const(wt.shape[0], 0.0)
        with self.grads():
            return self.V.conv2d_bn_act(t.reshape(B, 1, 1, -1), wt, self.const(wt.shape[0], 1.0), shift, 1, 0, relu, self.precision)

    def bn(self, t, m, relu, residual=None):
        if m.momentum is None or not m.track_running_stats:
            raise RuntimeError("%s.forward_autograd: BatchNorm2d with a momentum and running statistics only (the reference's)" % self.who)
        if not m.training:                         # a frozen BatchNorm (the module itself in eval() mode): running statistics read, nothing updated
            return self.V.batch_norm_eval(t, m.weight, m.bias, m.running_mean, m.running_var, m.eps, relu, residual)
        self._counters.append(m.num_batches_tracked)
        return self.V.batch_norm_train(t, m.weight, m.bias, m.running_mean, m.running_var, m.momentum, m.eps, relu, residual)[0]

    def pyramid(self, x_nchw, rp):
        """ResNetPyramids.forward in train() mode: x NCHW -> [x1..x4] NHWC."""
        stem = rp.conv1
        t = self.V.stem_conv3x3s2(x_nchw, stem.conv1_1.weight, True)                      # no BatchNorm behind conv1_1 (the reference's)
        t = self.bn(self.conv(t, stem.conv1_2), stem.bn_2, True)
        t = self.bn(self.bn(self.conv(t, stem.conv1_3), stem.bn1_3, True), rp.bn1, True)
        t = self.V.maxpool3x3s2(t)
        levels = []
        for li in range(1, 5):
            for blk in getattr(rp, "layer%d" % li):
                u = self.bn(self.conv(t, blk.conv1), blk.bn1, True)
                u = self.bn(self.conv(u, blk.conv2), blk.bn2, True)
                idn = self.bn(self.conv(t, blk.downsample[0]), blk.downsample[1], False) if blk.downsample is not None else t
                t = self.bn(self.conv(u, blk.conv3), blk.bn3, True, idn)
            levels.append(t)
        return levels

    def branch(self, seq, t, level, sizes):
        """feature{level}_upsamping: Conv2d + BatchNorm2d + ReLU triples, and UpsamplingBilinear2d to the size of the next finer pyramid level of
        this input (the sizes the inference program uses; the reference's literals are those of 240 x 320)."""
        mods = list(seq)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Conv2d):
                assert isinstance(mods[i + 1], nn.BatchNorm2d) and isinstance(mods[i + 2], nn.ReLU)
                t = self.bn(self.conv(t, m), mods[i + 1], True)
                i += 3
            elif isinstance(m, nn.UpsamplingBilinear2d):
                level -= 1
                t = self.V.upsample_bilinear_ac(t, sizes[level][0], sizes[level][1], False)
                i += 1
            else:
                raise TypeError(type(m))
        return t

    def decoder(self, module, levels):
        """z1 + z2 + z3 + z4 (in that order) of module.feature{1..4}_upsamping over the pyramid levels [x1..x4]."""
        sizes = {i + 1: (t.shape[1], t.shape[2]) for i, t in enumerate(levels)}
        z = None
        for b in (1, 2, 3, 4):
            zb = self.branch(getattr(module, "feature%d_upsamping" % b), levels[b - 1], b, sizes)
            z = zb if z is None else self.V.add_rows(z, zb, False)
        return z

    def finish(self):
        if self._counters:                                                                # (none: every BatchNorm of the pass was frozen)
            torch._foreach_add_(self._counters, 1)                                        # every num_batches_tracked, one launch


def begin(module, tensors, precision, grad_precision=0):
    """How every forward_autograd opens, after its own shape checks: refuse CPU tensors, eval() mode, a precision without a backward and a
    grad_precision other than 0 / 2, and only then mark the module's folded inference weights stale and hand out the pass's Walk, whose convs (and
    DORN's Linear) run inside torch_ops.grad_precision(grad_precision); the stem and the heads, with backward kernels of their own, stay fp32."""
    who = type(module).__name__
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("%s runs on the GPU only: there is no CPU/eager fallback" % who)
    if not module.training:
        raise RuntimeError("%s.forward_autograd is the train() mode forward; call .train() (eval(): forward)" % who)
    walk = Walk(who, tensors[0].device, precision, grad_precision)
    module._autograd_dirty = True
    return walk
