"""Training steps of the two networks on the GPU: the depth-completion network (BASELINE configs[4]) and, with
`SurfaceNormalTrainer` at the end of this file, the surface-normal network.  Both share `_TrainerBase`; the text below describes the depth step.

`DepthCompletionTrainer(cnn, learning_rate).step(image, normal, depth_in, depth_gt)` is the body of the reference's
`ImageNetworkRunInterface._run_training_iteration` (network_run.py:231-254) for `self.cnn = ModifiedFPN`:

    cnn.train()                       BatchNorm on batch statistics, running statistics updated (momentum 0.1)
    outputs = cnn(image, normals, depth_enriched)          (the three inputs are what `_call_cnn`, main.py:261-298, feeds the network;
                                                            they do not depend on the trained parameters)
    loss = L1Loss(sum)(pred[gt > 0], gt[gt > 0]) / (H*W)   network_run.py:163-173
    loss.backward(); Adam(cnn.parameters(), lr).step()      network_run.py:228-229, 249-250

Everything numeric is a libvidc.so kernel: forward convs = the inference MFMA kernel (csrc/conv_mfma.hip) with the raw bias instead of a
folded BatchNorm, data gradients = the same kernel on flipped/transposed weights, weight gradients / BatchNorm / pooling / upsampling /
head / loss / Adam = csrc/train.hip.  PyTorch provides device memory, the parameter containers (the module keeps its reference
state_dict layout; parameters and their .grad become views of two flat buffers) and, across GPUs, `torch.distributed.all_reduce` of
the flat gradient buffer (RCCL): frames shard over ranks, every rank normalises BatchNorm over ITS frames (what the reference's
DataParallel replicas do as well) and gradients are SUMMED, which equals the reference's single loss over the whole batch.
There is no CPU path.  Arithmetic: exact fp32 MFMA products in all three conv passes (the reference's arithmetic: gradients sit at
the reference's own fp32 noise floor).  VIDC_TRAIN_PRECISION=bf16x3 runs the three conv passes in the split-bf16 3-pass mode of
the inference path (~2^-16 per product; 1.5x the step rate) and VIDC_TRAIN_PRECISION=bf16 in plain bf16 with fp32 accumulation -- the
arithmetic BASELINE configs[4] names (2x; fp32 master weights, BatchNorm, loss and Adam in all modes).  Both keep the loss to 4-6
digits; individual gradient tensors move by percents of their scale (flipped ReLU gates propagate through the train-mode BatchNorms):
throughput modes, not the parity mode (tests/test_training.py states their bars)."""
import ctypes as C
import json
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import engine
from .networks.fpn_decoder import _BRANCH_PLAN

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
PYRAMIDS = ("resnet_rgb", "resnet_normal", "resnet_depth")      # the three ResNet-101 pyramids of ModifiedFPN (depth_completion.py:75-77)


def _keys(key):
    """A parameter-name prefix, or one per group of a grouped launch (the same layer of the three pyramids)."""
    return (key,) if isinstance(key, str) else tuple(key)


def _cat(p, suffix):
    return tuple(q + suffix for q in _keys(p)) if not isinstance(p, str) else p + suffix


class Act:
    """An activation: NHWC rows `t` (B,H,W,C view, possibly a channel slice of a wider buffer) + its gradient (same geometry)."""
    __slots__ = ("t", "grad", "bf", "grad_bf", "grad_t", "conv_out", "no_f32_grad", "stats")      # bf / grad_bf: bf16 operand copies (dense rows) written by the producing kernel
    # grad_t: (tensor, Mp) -- the gradient transposed as bf16 rows [C][Mp], written by the BatchNorm backward behind a conv (conv_out): the
    # left operand of that conv's weight-gradient GEMM

    def __init__(self, t):
        self.t, self.grad, self.bf, self.grad_bf, self.grad_t, self.conv_out = t, None, None, None, None, False
        self.stats = None             # conv output in the plain-bf16 mode: per-32-row-block channel sums written by the conv's epilogue (VIDC_STATS_OUT)
        self.no_f32_grad = False      # conv output whose conv reads dY only through grad_bf / grad_t: the BatchNorm backward skips the fp32 form

    @property
    def ld(self):
        return self.t.stride(2)

    @property
    def rows(self):
        return self.t.shape[0] * self.t.shape[1] * self.t.shape[2]


_TRAIN_TUNING = None


def training_table():
    """Per-shape [tile_fp32, splitk_fp32, tile_bf16x3, splitk_bf16x3] of the training step's conv launches (forward, dgrad and the
    wgrad GEMMs), measured on MI355X by tools/autotune_train.py.  VIDC_TRAIN_TUNING=0 ignores it (cost-model plan)."""
    global _TRAIN_TUNING
    if _TRAIN_TUNING is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_tuning.json")
        use = os.environ.get("VIDC_TRAIN_TUNING", "1") != "0" and os.path.exists(path)
        _TRAIN_TUNING = json.load(open(path)) if use else {}
    return _TRAIN_TUNING


def _ld(t):
    return t.stride(2)


def build_segment_table(named_sizes, param_groups=None, weight_decay=0.0):
    """The segment table of csrc/optim.hip (include/vidc.h) for a flat buffer: `named_sizes` is [(name, numel)] in the buffer's order (the
    trainer's `named`, whichever layout it chose -- in "grouped" the three pyramids interleave per name, so a pyramid's group becomes many
    segments), `param_groups` a sequence of (match, options): match a name prefix or a callable name -> bool, the first match wins; options
    may hold "lr_scale", "weight_decay", "frozen".  A parameter that matches nothing takes lr_scale 1, `weight_decay`, not frozen.
    Adjacent tensors with equal settings share a segment.  Returns (begin, lr_scale, weight_decay, flags): begin has one entry more than the
    others, begin[0] = 0, begin[-1] = the buffer's length; flags bit 0 = frozen.  A pure function (no device, no trainer)."""
    groups = []
    for match, options in (param_groups or ()):
        unknown = set(options) - {"lr_scale", "weight_decay", "frozen"}
        if unknown:
            raise ValueError("param_groups: unknown option(s) %s (lr_scale, weight_decay, frozen)" % sorted(unknown))
        if not (isinstance(match, str) or callable(match)):
            raise ValueError("param_groups: a match is a name prefix or a callable name -> bool, got %r" % (match,))
        groups.append((match, options))
    begin, lr_scale, decay, flags = [0], [], [], []
    o = 0
    for name, numel in named_sizes:
        options = next((opt for match, opt in groups if (name.startswith(match) if isinstance(match, str) else match(name))), {})
        setting = (float(options.get("lr_scale", 1.0)), float(options.get("weight_decay", weight_decay)), int(bool(options.get("frozen", False))))
        if numel <= 0:
            continue
        if lr_scale and setting == (lr_scale[-1], decay[-1], flags[-1]):
            begin[-1] = o + numel
        else:
            lr_scale.append(setting[0]); decay.append(setting[1]); flags.append(setting[2])
            begin.append(o + numel)
        o += numel
    return begin, lr_scale, decay, flags


class GradientBuckets:
    """The flat gradient buffer cut into buckets for the cross-rank SUM (one collective per bucket, ~64 MB each: large enough that a
    ring all-reduce over xGMI runs at link speed, small enough to start before the whole backward has finished if overlapped).

    compress="bf16" (DepthCompletionTrainer: VIDC_TRAIN_GRAD_BF16=1): every bucket travels rounded to bf16 -- 0.62 GB instead of
    1.24 GB per step for ModifiedFPN, i.e. ~7 instead of ~14 ms on a ring at 153 GB/s per xGMI link -- and is widened back into the
    fp32 buffer before Adam reads it (vidc_grad_narrow_bf16 / vidc_grad_widen_bf16; the SUM itself is RCCL's, in bf16).  An opt-in:
    the reference's DataParallel sums its replicas' gradients in fp32 (network_run.py:97-99)."""

    def __init__(self, n_elements, bucket_elements=16 * 1024 * 1024, compress=None):
        self.ranges = [(a, min(n_elements, a + bucket_elements)) for a in range(0, n_elements, bucket_elements)]
        self.compress = compress
        self._narrow = None            # persistent bf16 image of the flat buffer (allocated on first use)

    def all_reduce(self, flat):
        for w in self.all_reduce_async(flat):
            w()
        return flat

    def all_reduce_async(self, flat, lo=0, hi=None):
        """Starts the SUM over ranks of flat[lo:hi], bucket by bucket, and returns the completion callbacks (call every one before the
        data is used).  RCCL: the collectives run on the process group's own stream, after the work already enqueued on the current
        stream, and overlap whatever is enqueued next -- the decoder's gradients travel while the pyramids' backward runs
        (DepthCompletionTrainer.step).  gloo (trying the N > 1 path on a box without a second GPU): through the host, synchronous."""
        import torch.distributed as dist
        from .sharding import collectives_active
        if not collectives_active():
            return []
        hi = flat.numel() if hi is None else hi
        stage = dist.get_backend() == "gloo" and flat.is_cuda
        bf16 = self.compress == "bf16" and flat.is_cuda
        if bf16 and (self._narrow is None or self._narrow.numel() != flat.numel() or self._narrow.device != flat.device):
            self._narrow = torch.empty(flat.numel(), dtype=torch.bfloat16, device=flat.device)
        waits = []
        for a, b in self.ranges:
            a, b = max(a, lo), min(b, hi)
            if a >= b:
                continue
            if bf16 and a % 8 and b - a > 8:      # a range that starts off the kernels' 16-byte grid (the decoder's first parameter): its first
                a_up = a + 8 - a % 8              # few elements travel as they are, in fp32
                head = flat[a:a_up]
                if stage:
                    h = head.cpu()
                    dist.all_reduce(h, op=dist.ReduceOp.SUM)
                    head.copy_(h)
                else:
                    waits.append(dist.all_reduce(head, op=dist.ReduceOp.SUM, async_op=True).wait)
                a = a_up
            if bf16 and a % 8 == 0:
                src, nb = flat[a:b], self._narrow[a:b]
                L.check(L.lib().vidc_grad_narrow_bf16(L.ptr(src), L.ptr(nb), b - a, L.current_stream()), "grad narrow")
                if stage:
                    h = nb.cpu()
                    dist.all_reduce(h, op=dist.ReduceOp.SUM)
                    nb.copy_(h)
                    L.check(L.lib().vidc_grad_widen_bf16(L.ptr(nb), L.ptr(src), b - a, L.current_stream()), "grad widen")
                else:
                    work = dist.all_reduce(nb, op=dist.ReduceOp.SUM, async_op=True)

                    def done(work=work, nb=nb, src=src, n=b - a):
                        work.wait()               # (the current stream waits for the collective; the widening pass follows on it)
                        L.check(L.lib().vidc_grad_widen_bf16(L.ptr(nb), L.ptr(src), n, L.current_stream()), "grad widen")
                    waits.append(done)
            elif stage:
                h = flat[a:b].cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM)
                flat[a:b].copy_(h)
            else:
                waits.append(dist.all_reduce(flat[a:b], op=dist.ReduceOp.SUM, async_op=True).wait)
        return waits


class _TrainerBase:
    """What the two trainers share: the flat parameter / gradient / Adam-moment buffers, the recording ops (conv, bn, add, maxpool, upsample, the
    ResNet-101 pyramid and the decoder branches -- each launches its forward and records its backward on the tape), weight packing, the tape and
    its stream lanes, the head, `step` with its graph capture / replay and the Adam step.  A subclass names its pyramids (`pyramid_names`) and
    writes the network walk (`forward`: three inputs) and the loss (`loss_and_backward`: the prediction and the remaining inputs).

    Build the trainer AFTER `torch.distributed.init_process_group` (and after the network is on its GPU): the flat layout of parameters, gradients, Adam
    moments and BatchNorm running statistics is chosen here (`self.layout`: "grouped" = the three pyramids interleaved per parameter name, the multi-rank
    default of the depth trainer; "per_pyramid" otherwise) and every launch of the step addresses tensors as base + offset into those buffers.  A later
    `cnn.to()` / `.float()` / `.cuda()` that rebinds `p.data` is caught at the next `step()` (`_check_bindings`), not silently read through stale pointers.

    Optimizer options (csrc/optim.hip; all of it on the device, nothing is read back, the step stays asynchronous).  With every one at its
    default and no accumulation window open the step issues exactly the launches it issued before these existed (`vidc_adam_step`).
      weight_decay, decoupled_weight_decay   torch.optim.Adam(weight_decay=...)'s L2 term, or with decoupled_weight_decay torch.optim.AdamW's
      max_grad_norm       torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) on the (rank-summed, window-summed) gradient of the
                          non-frozen parameters.  The norm pass runs exactly when max_grad_norm is not None, and `last_grad_norm` (a 0-dim
                          fp64 device tensor, the norm before clipping; None otherwise) is then refreshed by every optimizer step;
                          float("inf") measures without clipping.  Across ranks every rank holds the summed gradient: no extra collective.
      param_groups        a sequence of (match, options): a name prefix or a callable name -> bool, the first match wins; options
                          "lr_scale", "weight_decay", "frozen" (`build_segment_table`).  A frozen parameter keeps its value and moments bit
                          for bit and is left out of the norm; its gradient is still computed.
      accumulate_mean     `backward_only(*ins)` runs a step's forward + backward and adds the gradient to a window (no all-reduce, no update);
                          the next `step` closes the window: the update sees the SUM of the window's gradients -- what summing over ranks
                          already means for the depth loss, which divides by the constant H*W: k micro-batches of B frames are one batch of
                          k B -- or with accumulate_mean their mean.  The normal loss divides by N, the unmasked pixels of ITS batch, so
                          each micro-batch's gradient is already an average and a window of k usually wants the mean (the sum is a k times
                          larger step before Adam's normalisation has adapted, and k times the norm that max_grad_norm sees).
    `lr` stays a plain attribute passed by value: a schedule is an assignment between steps."""

    pyramid_names = PYRAMIDS

    def __init__(self, cnn, learning_rate=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None,
                 param_groups=None, accumulate_mean=False):
        if not torch.cuda.is_available():
            raise RuntimeError("%s needs a GPU: the HIP path has no CPU fallback" % type(self).__name__)
        self.cnn = cnn
        self.lr, self.betas, self.eps = float(learning_rate), betas, float(eps)
        self.weight_decay, self.decoupled_weight_decay = float(weight_decay), bool(decoupled_weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.param_groups = list(param_groups or ())
        self.accumulate_mean = bool(accumulate_mean)
        if self.weight_decay < 0 or (self.max_grad_norm is not None and not self.max_grad_norm > 0):
            raise ValueError("weight_decay must be >= 0 and max_grad_norm > 0 (float('inf'): measure the norm, never clip)")
        build_segment_table([], self.param_groups)      # (refuses malformed groups before any parameter is rebound)
        self.named = [(k, p) for k, p in cnn.named_parameters()]
        # Grouped pyramids (round 5, VIDC_TRAIN_GROUPED=0 switches back to one launch chain per pyramid): the same layer of the three
        # pyramids runs as ONE launch with three groups -- forward conv, data gradient, weight-gradient GEMM -- and ONE BatchNorm launch over
        # the 3 x C channels of the grouped tensor, as the inference frame program has always done.  A group selects base pointers only, so
        # the three layers' parameters (and gradients, Adam moments, BatchNorm running statistics) are laid out next to each other in the
        # flat buffers: [rgb | normal | depth] per parameter name.  Values, gradients and the all-reduced sums are what they were.
        # (the grouped weight-gradient GEMM writes the three .grad tensors in place; the A/B switch VIDC_TRAIN_WGRAD_INPLACE=0 -- staging
        #  buffer + permute, tap-major operand rows -- therefore runs the per-pyramid chains)
        # Default ("auto"): grouped + ONE stream when the step runs across ranks, three per-pyramid stream lanes on a single rank.  Measured
        # (MI355X, batch 8, bf16, profiles/r5_train_grouped_ab.txt): grouped = 1252 launches / 27.8 ms of kernel time per step instead of
        # 3258 / 42.0 ms, but as ONE dependency chain (27.3-27.5 ms per step) against 25.9 ms for the three lanes, whose launch latencies
        # hide under each other -- on this runtime kernels of different streams fill each other's gaps, they do not add throughput.
        # Across ranks the step is cut into two graphs around the decoder's all-reduce, and there the three-lane form falls into the
        # runtime's slow regime above 4 hardware queues (50.4 against 27.4 ms at 8 queues) while the single-stream grouped chain
        # does not care (27.8 / 28.4 ms at 4 / 8 queues): the multi-rank default must not depend on a queue count nobody controls.
        mode = os.environ.get("VIDC_TRAIN_GROUPED", "auto")
        want = self._distributed() if mode == "auto" else mode == "1"
        self.grouped = (want and os.environ.get("VIDC_TRAIN_WGRAD_INPLACE", "1") == "1" and
                        len(self.pyramid_names) > 1 and all(hasattr(cnn, pn) for pn in self.pyramid_names))
        if self.grouped:
            by_name = dict(self.named)
            first = self.pyramid_names[0] + "."
            inter = []
            for k, _p in self.named:
                if k.startswith(first):
                    for pn in self.pyramid_names:
                        kk = pn + "." + k[len(first):]
                        inter.append((kk, by_name[kk]))
            seen = {k for k, _ in inter}
            self.named = inter + [(k, q) for k, q in self.named if k not in seen]
        dev = self.named[0][1].device
        if dev.type != "cuda":
            raise RuntimeError("move the network to the GPU before building the trainer")
        self.device = dev
        n = sum(p.numel() for _, p in self.named)
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.param, self.grad = {}, {}
        o = 0
        for k, p in self.named:            # parameters and gradients become views of the flat buffers (one Adam launch, bucketed all-reduce)
            k_n = p.numel()
            self.flat_p[o:o + k_n].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[o:o + k_n].view(p.shape)
            p.grad = self.flat_g[o:o + k_n].view(p.shape)
            self.param[k], self.grad[k] = p.data, p.grad
            o += k_n
        self.buf = {k: b for k, b in cnn.named_buffers()}
        if self.grouped:      # BatchNorm running statistics of the three pyramids: the same interleaved order, in a flat buffer of their own
            first = self.pyramid_names[0] + "."
            fl = [k for k in self.buf if k.startswith(first) and self.buf[k].dtype == torch.float32]
            tot = sum(self.buf[k].numel() for k in fl) * len(self.pyramid_names)
            self.flat_b = torch.empty(tot, dtype=torch.float32, device=dev)
            o = 0
            for k in fl:
                for pn in self.pyramid_names:
                    b = self.buf[pn + "." + k[len(first):]]
                    self.flat_b[o:o + b.numel()].copy_(b.detach().reshape(-1))
                    b.data = self.flat_b[o:o + b.numel()].view(b.shape)
                    o += b.numel()
        self._adjacent = {}
        self.layout = "grouped" if self.grouped else "per_pyramid"      # (exported with `flat_state()`: moments of one layout are not another's)
        self._bind_probe = [(self.named[i][1], self.param[self.named[i][0]].data_ptr(), self.grad[self.named[i][0]].data_ptr()) for i in (0, len(self.named) - 1)]
        if self.grouped:
            fb = [k for k in self.buf if self.buf[k].dtype == torch.float32 and any(k.startswith(pn + ".") for pn in self.pyramid_names)]
            self._bind_probe += [(self.buf[k], self.buf[k].data_ptr(), None) for k in (fb[0], fb[-1])] if fb else []
        self.buckets = GradientBuckets(n, compress=("bf16" if os.environ.get("VIDC_TRAIN_GRAD_BF16", "0") == "1" else None))
        # the decoder's parameters (feature*_upsamping, feature_concat) form the tail of the flat buffers (named_parameters order): their
        # gradients are complete when the decoder's backward is, long before the pyramids' -- they are all-reduced while those still run
        offs = {k: int((self.grad[k].data_ptr() - self.flat_g.data_ptr()) // 4) for k, _ in self.named}
        dec = [offs[k] for k, _ in self.named if k.startswith("feature")]
        self._dec_off = min(dec) if dec and all(k.startswith("feature") for k, _ in self.named if offs[k] >= min(dec)) else n
        self.step_count = 0
        # the optimizer options as the kernels take them: the segment table (None: one segment at the defaults), the norm record and the window
        begin, lr_scale, decay, flags = build_segment_table([(k, p.numel()) for k, p in self.named], self.param_groups, self.weight_decay)
        self._seg = None
        if (lr_scale, decay, flags) != ([1.0], [0.0], [0]):
            self._seg = (len(lr_scale), torch.tensor(begin, dtype=torch.int64, device=dev), (C.c_longlong * len(begin))(*begin),
                         torch.tensor(lr_scale, dtype=torch.float32, device=dev), torch.tensor(decay, dtype=torch.float32, device=dev),
                         torch.tensor(flags, dtype=torch.int32, device=dev))
        self._any_frozen = any(flags)
        self._options_on = self._seg is not None or self.max_grad_norm is not None
        self._norm_record = self._norm_scratch = self.last_grad_norm = None
        if self.max_grad_norm is not None:
            self._norm_record = torch.zeros(2, dtype=torch.float64, device=dev)       # vidc_grad_sqnorm's [total norm, gradient factor]
            self._norm_scratch = torch.empty(L.lib().vidc_grad_sqnorm_scratch_bytes(n), dtype=torch.uint8, device=dev)
            self.last_grad_norm = self._norm_record[0]
        self.flat_acc, self._window = None, 0      # gradient sum of the open accumulation window and its number of micro-steps (0: closed)
        self._ones, self._zeros, self._packed, self._scratch, self._nbt = {}, {}, {}, {}, []
        self._gemm_ws = {}          # split-K workspace per stream lane (lane 0 = the caller's stream)
        self._cur = 0               # stream lane the ops being recorded / replayed run on (0 = main, 1..3 = the three pyramids, 1..4 = the decoder branches)
        self._lanes = None
        self.n_lanes = int(os.environ.get("VIDC_TRAIN_STREAMS", "1" if self.grouped else "3"))      # (grouped: the decoder's four branches stay on the caller's stream too)
        self._pack_items, self._pack_table, self._packed_fresh = [], None, False
        self.use_graph = os.environ.get("VIDC_TRAIN_GRAPH", "1") != "0"
        self._graphs, self._graph_seen = {}, {}
        # Opt-in experiment (VIDC_TRAIN_WGRAD_STREAM=1), measured SLOWER and therefore off: dW of a conv (two operand transposes, a GEMM, a
        # permute, the bias column sum -- 4-5 launches) depends on dY only and nothing depends on it until Adam, so it can run on a side
        # stream of its lane while the lane goes on with the data gradient (in the captured graph: a parallel branch per conv), taking a
        # third of the launches out of a pyramid's dependency chain.  Round 3, batch 8, same box, identical losses: 41.6 ms per step
        # against 32.6 in bf16, 80.4 against 71.6 in fp32 -- ~340 extra fork / join edges per step cost more than the shorter chain
        # saves (the same finding as for side streams inside the inference graphs).
        self.wgrad_side = os.environ.get("VIDC_TRAIN_WGRAD_STREAM", "0") == "1"
        # Round-3 launch reductions, each bit-identical to the form it replaces; the switches exist for the A/B runs and the tests:
        # dY^T of a conv written by the BatchNorm backward that produces dY; the weight-gradient GEMM writing .grad in place (channel-major
        # operand rows); the residual add writing the block output's bf16 operand copy.
        self.dyt_fused = os.environ.get("VIDC_TRAIN_DYT_FUSED", "1") == "1"
        self.wgrad_inplace = os.environ.get("VIDC_TRAIN_WGRAD_INPLACE", "1") == "1"
        self.add_bf16 = os.environ.get("VIDC_TRAIN_ADD_BF16", "1") == "1"
        self.bn_add_fused = os.environ.get("VIDC_TRAIN_BN_ADD_FUSED", "1") == "1"   # Bottleneck tail relu(bn3(.) + identity) inside bn3's apply pass
        self.skip_f32_dy = os.environ.get("VIDC_TRAIN_SKIP_F32_DY", "1") == "1"    # the BatchNorm backward writes no fp32 dY where only the bf16 forms are read
        self.xt_from_bf16 = os.environ.get("VIDC_TRAIN_XT_BF16", "1") == "1"      # 1x1 convs: the wgrad GEMM's right operand transposed from the bf16 copy
        # Round 4: the train-mode BatchNorm behind a conv takes its per-channel sums from the conv's epilogue (VIDC_STATS_OUT, plain-bf16 mode)
        # instead of a partial-sum pass of its own over the conv output: one launch and one read of the tensor less per conv + BatchNorm.
        self.conv_stats = os.environ.get("VIDC_TRAIN_CONV_STATS", "1") == "1"
        self.conv_stats_max_m = int(os.environ.get("VIDC_TRAIN_CONV_STATS_MAX_M", str(1 << 30)))
        if "VIDC_TRAIN_BN_FOLD" in os.environ:   # (A/B runs) the BatchNorm chunk sums reduced in the consumer's prologue (default) or by a launch of their own
            L.lib().vidc_train_bn_fold(int(os.environ["VIDC_TRAIN_BN_FOLD"] != "0"))
        self._wgrad_streams, self._wgrad_used = {}, []
        self._retired = []          # outgrown scratch / workspace buffers that captured graphs still address (see _retire)
        self._keepalive = []        # backward closures already run in the current _run_tape, kept until the stream lanes have joined
        self.tune_hook = None      # tools/autotune_train.py: called with every conv descriptor before it is planned
        self.precision = {"fp32": L.PREC_FP32, "bf16x3": L.PREC_BF16X3, "bf16": L.PREC_BF16}[os.environ.get("VIDC_TRAIN_PRECISION", "fp32")]
        self.last_loss = None

    # ---- small helpers ------------------------------------------------------------------------------------------------------
    def _const(self, store, n, value):
        if n not in store:
            store[n] = torch.full((n,), value, dtype=torch.float32, device=self.device)
            torch.cuda.current_stream().synchronize()     # made on one stream lane, read by all of them from now on
        return store[n]

    def _scratch_bytes(self, nbytes):
        sc = self._scratch.get(self._cur)                 # one scratch per stream lane: the lanes run concurrently
        if sc is None or sc.numel() < nbytes:
            self._retire(sc)
            sc = self._scratch[self._cur] = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
        return sc

    def _retire(self, t):
        """A scratch / split-K workspace that is being replaced by a larger one.  Captured step graphs of OTHER input shapes hold its raw
        address (BN / column-sum partials, split-K partial tiles and their ticket counters), so it must never go back to the allocator
        while such a graph can still be replayed: it is parked for the lifetime of the trainer (the graphs keep using it; new eager
        steps and new captures use the larger buffer)."""
        if t is not None and self._graphs:
            self._retired.append(t)

    def _record(self, fn):
        fn._lane = self._cur
        self.tape.append(fn)

    def _beside(self, fn):
        """Runs `fn` (launches that nothing on the current lane waits for before the end of the backward) on the lane's side stream, with
        its own scratch / split-K workspace key; `_join_wgrad` makes the main stream wait for all of them."""
        if not self.wgrad_side:
            fn()
            return
        lane = self._cur
        cur = torch.cuda.current_stream()
        side = self._wgrad_streams.get(lane)
        if side is None:
            side = self._wgrad_streams[lane] = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)                     # dY (and its ReLU mask) are complete on the lane
        self._keepalive.append(fn)                # fn owns tensors of the LANE's allocator pool (the masked dY): alive until the join
        self._cur = lane + 8
        try:
            with torch.cuda.stream(side):
                fn()
        finally:
            self._cur = lane
        if side not in self._wgrad_used:
            self._wgrad_used.append(side)

    def _join_wgrad(self, main):
        for side in self._wgrad_used:
            main.wait_stream(side)
        self._wgrad_used = []

    def _lane_streams(self):
        if self._lanes is None:
            self._lanes = [torch.cuda.Stream(device=self.device) for _ in range(4)]
        return self._lanes

    def _train_scratch(self, M, Cc):
        return self._scratch_bytes(L.lib().vidc_train_scratch_bytes(M, Cc))

    def _empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    # ---- conv: forward, dgrad, wgrad --------------------------------------------------------------------------------------------
    def _conv_call(self, x_t, w_packed, shift, y_t, kh, kw, stride, pad, relu, accumulate, x_bf=None, stats=None, groups=1):
        """One launch of the inference conv kernel.  In bf16x3 mode the activations are split here (one extra pass over x); `w_packed`
        must already be in the matching format (`_pack`).  groups = G > 1: x_t / y_t hold G groups as channel slices ([.., G*cin] /
        [.., G*cout]), w_packed the G packed weights back to back; `shift` ([cout]) is shared by the groups."""
        B, H, W, cin = x_t.shape
        _, Ho, Wo, cout = y_t.shape
        G = groups
        ldx = _ld(x_t)
        if self.precision == L.PREC_BF16X3:
            xs = self._empty(B, H, W, cin)
            L.check(L.lib().vidc_split_bf16x3(L.ptr(x_t), L.ptr(xs), B * H * W, cin, ldx, L.current_stream()), "split")
            x_t, ldx = xs, cin
        elif self.precision == L.PREC_BF16:      # plain bf16 rows; the descriptor counts two channels per element (include/vidc.h)
            if (cin // G) % 64:
                raise RuntimeError("bf16 training needs conv input channels in multiples of 64 (got %d)" % (cin // G))
            xs = x_bf                             # the producer wrote the bf16 copy already (bn / bn backward)
            if xs is not None and tuple(xs.shape) != (B, H, W, cin // 2):
                raise RuntimeError("bf16 operand copy of shape %s for an activation of shape %s" % (tuple(xs.shape), (B, H, W, cin)))
            if xs is None:
                xs = self._empty(B, H, W, cin // 2)
                L.check(L.lib().vidc_cast_bf16(L.ptr(x_t), L.ptr(xs), B * H * W, cin, ldx, L.current_stream()), "cast")
            x_t, ldx = xs, cin                    # (dense rows of cin channels)
        d = L.conv_desc(B, H, W, cin // G, cout // G, kh, kw, stride, pad, groups=G, Ho=Ho, Wo=Wo, ldx=ldx, ldy=_ld(y_t), precision=self.precision,
                        x=L.ptr(x_t), w=L.ptr(w_packed), y=L.ptr(y_t), scale1=L.ptr(self._const(self._ones, cout // G, 1.0)), shift1=L.ptr(shift),
                        shared_affine=True, relu1=relu, accumulate=accumulate, stats_out=L.ptr(stats))
        self._plan(d, "conv")
        L.check(L.lib().vidc_conv2d_bn_act(C.byref(d), L.current_stream()), "conv")

    def _plan(self, d, role):
        """Tile / split-K of one launch: the table measured on MI355X at the training shapes (train_tuning.json, tools/autotune_train.py:
        [tile, splitk] per arithmetic mode), else the planner's cost model.  Split-K partial sums go through one persistent workspace
        (ticket counters at its head, zeroed once; the last workgroup of a tile resets its ticket)."""
        lib = L.lib()
        if not (self.tune_hook is not None and self.tune_hook(d, role)):      # (a hook that returns True has set tile / splitk itself)
            ent, p = training_table().get(engine.conv_signature(d)), 2 * d.precision
            tiling = (ent[p], ent[p + 1]) if ent is not None and len(ent) > p + 1 and ent[p] else None
            L.plan(d, tiling)
            if tiling is None and role == "conv":
                d.splitk = 1
        need = lib.vidc_conv2d_workspace_bytes(C.byref(d))
        if need:
            ws = self._gemm_ws.get(self._cur)
            if ws is None or ws.numel() * 4 < need:
                self._retire(ws)
                ws = self._gemm_ws[self._cur] = torch.zeros(int(need // 4 * 1.5) + 16, dtype=torch.float32, device=self.device)
            d.workspace = L.ptr(ws)

    def _pack(self, key, kind, w):
        """Packed weights of conv `key` for the forward ('f') or the dgrad ('d': kernel flipped, channels transposed) launch, in the
        trainer's arithmetic mode.  The parameters move every step: `repack()` rebuilds every packed copy with one launch at the start of
        a forward; a conv met for the first time is packed here and joins the table."""
        keys = _keys(key)                      # (a tuple: the G packed copies back to back, what a grouped launch reads as w + g * w_gs)
        ent = self._packed.get((keys, kind))
        if ent is not None and self._packed_fresh:
            return ent[0]
        co, ci, kh, kw = w.shape
        if ent is None:
            n1 = co * ci * kh * kw // (2 if self.precision == L.PREC_BF16 else 1)
            buf = self._empty(n1 * len(keys))
            mine = []
            for g, k in enumerate(keys):
                wk = self.param[k + ".weight"] if len(keys) > 1 else w
                assert tuple(wk.shape) == (co, ci, kh, kw), k
                mine.append((wk, buf[g * n1:(g + 1) * n1], co, ci, kh, kw, (1 if kind == "d" else 0) | {L.PREC_FP32: 0, L.PREC_BF16X3: 2, L.PREC_BF16: 4}[self.precision]))
            self._pack_items += mine
            ent = self._packed[(keys, kind)] = (buf, mine)
            self._pack_table = None
        self._launch_pack(ent[1])
        return ent[0]

    def _launch_pack(self, items):
        table = (L.PackItem * len(items))()
        blocks = 0
        for t, (w, out, co, ci, kh, kw, kind) in zip(table, items):
            t.w, t.packed, t.Cout, t.Cin, t.KH, t.KW, t.kind, t.block_begin = L.ptr(w), L.ptr(out), co, ci, kh, kw, kind, blocks
            nb = L.lib().vidc_pack_item_blocks(co, ci, kh, kw, kind)
            if nb <= 0:
                raise RuntimeError("conv weight %dx%dx%dx%d cannot be packed for kind %d (K-side channels must fill whole 128-byte units)" % (co, ci, kh, kw, kind))
            blocks += nb
        dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        L.check(L.lib().vidc_pack_conv_weights_batched(L.ptr(dev), len(items), blocks, L.current_stream()), "pack")
        return dev, blocks

    def repack(self):
        """One launch re-packs every conv weight seen so far (forward and dgrad copies) from the current parameters."""
        if self._pack_items:
            if self._pack_table is None:
                dev, blocks = self._launch_pack(self._pack_items)
                self._pack_table = (dev, blocks, len(self._pack_items))
            else:
                dev, blocks, n = self._pack_table
                L.check(L.lib().vidc_pack_conv_weights_batched(L.ptr(dev), n, blocks, L.current_stream()), "pack")
        self._packed_fresh = True

    def _check_bindings(self):
        """O(1) per step: the first and last parameter (and, grouped, running statistic) still live where the flat buffers put them.  `cnn.to()`,
        `.float()`, `.cuda()` or a `load_state_dict(assign=True)` after construction rebind `.data`; the captured graphs and the grouped launches
        (base + g * numel) would then read the old storage."""
        for t, p_ptr, g_ptr in self._bind_probe:
            if t.data_ptr() != p_ptr or (g_ptr is not None and (t.grad is None or t.grad.data_ptr() != g_ptr)):
                raise RuntimeError("%s: a parameter / buffer of the network was rebound after the trainer was built (layout %r); "
                                   "build a new trainer after moving or casting the network" % (type(self).__name__, self.layout))

    def flat_state(self):
        """Optimizer state for a checkpoint: the flat Adam moments with the layout they belong to and the parameter order that defines the offsets,
        and (a record for whoever reads the checkpoint; a trainer's options are its constructor's) the optimizer options they were made under."""
        if self._window:
            raise RuntimeError("flat_state(): an accumulation window of %d micro-step(s) is open; close it with step() first (its gradient sum is not "
                               "part of the state)" % self._window)
        begin, lr_scale, decay, flags = build_segment_table([(k, p.numel()) for k, p in self.named], self.param_groups, self.weight_decay)
        options = {"weight_decay": self.weight_decay, "decoupled_weight_decay": self.decoupled_weight_decay, "max_grad_norm": self.max_grad_norm,
                   "accumulate_mean": self.accumulate_mean, "segments": {"begin": begin, "lr_scale": lr_scale, "weight_decay": decay, "flags": flags}}
        return {"layout": self.layout, "order": [k for k, _ in self.named], "m": self.m, "v": self.v, "step_count": self.step_count, "options": options}

    def load_flat_state(self, st):
        """(`st["options"]`, absent from states saved before the options existed, is not applied: the options are this trainer's constructor's.)"""
        if st["layout"] != self.layout or list(st["order"]) != [k for k, _ in self.named]:
            raise RuntimeError("optimizer state of layout %r / another parameter order cannot be loaded into a trainer of layout %r (build the trainer under the "
                               "same VIDC_TRAIN_GROUPED setting and process-group state)" % (st["layout"], self.layout))
        self.m.copy_(st["m"]); self.v.copy_(st["v"]); self.step_count = int(st["step_count"])

    def _adjacent_base(self, store, keys, suffix):
        """The G tensors `store[k + suffix]` of a grouped layer as ONE contiguous run (group g at base + g * numel): the first one's
        tensor after a check, once per layer, that the flat layout really put them next to each other."""
        t0 = store[keys[0] + suffix]
        if len(keys) > 1:
            ck = (id(store), keys, suffix)
            if ck not in self._adjacent:
                for g, k in enumerate(keys):
                    t = store[k + suffix]
                    if t.shape != t0.shape or t.data_ptr() != t0.data_ptr() + 4 * g * t0.numel():
                        raise RuntimeError("grouped training: %s%s of the pyramids are not adjacent in the flat buffers" % (k, suffix))
                self._adjacent[ck] = True
        return t0

    def _wgrad_fits(self, geom, G=1):
        """Whether `_wgrad_gemm` takes this shape (else the direct pixel-reduction kernel runs, which reads the fp32 dY)."""
        B, H, W, ci, Ho, Wo, co, kh, kw, stride, pad = geom
        if os.environ.get("VIDC_WGRAD", "gemm") != "gemm":
            return False
        taps, M = kh * kw, B * Ho * Wo
        bf16 = self.precision == L.PREC_BF16
        Mp = (M + 63) // 64 * 64 if bf16 else (M + 31) // 32 * 32
        e = 2 if bf16 else 1
        return not (taps * ci * Mp * 4 // e >= (1 << 31) or G * co * Mp // e >= (1 << 29) or ci % 32 or co % 4)

    def _wgrad_gemm(self, g, x, key, geom, g_t=None):
        """dW through the conv kernel: dW[co][ci][tap] = sum over pixels of dY^T[co][m] * Xt[ci*taps + tap][m] is the 1x1 case of
        vidc_conv2d_bn_act with the rows of dY^T as activations and the rows of Xt (the transposed im2col of x, channel-major) as weights
        -- LDS-tiled, split-K, at several times the rate of the direct pixel-reduction kernel (vidc_conv_wgrad, kept for shapes beyond the
        32-bit limits of the conv kernel) -- and its output is the parameter's .grad in place.  g_t: dY^T if the BatchNorm backward has
        written it already.  Returns False when the shape does not fit."""
        B, H, W, ci, Ho, Wo, co, kh, kw, stride, pad = geom          # ci, co: per group
        keys = _keys(key)
        G = len(keys)
        if not self._wgrad_fits(geom, G) or (G > 1 and not self.wgrad_inplace):
            return False
        lib, st = L.lib(), L.current_stream()
        taps, M = kh * kw, B * Ho * Wo
        bf16 = self.precision == L.PREC_BF16
        Mp = (M + 63) // 64 * 64 if bf16 else (M + 31) // 32 * 32
        e = 2 if bf16 else 1                     # pixels per 4-byte element of an operand row
        # grouped: the rows of both operands are channel-major over ALL groups' channels, i.e. group g's rows are a contiguous run
        xt = self._empty(G * taps * ci, Mp // e)
        split = {L.PREC_FP32: 0, L.PREC_BF16X3: 1, L.PREC_BF16: 2}[self.precision]      # operands written in the GEMM's format directly
        if g_t is not None and bf16 and g_t[1] == Mp and g_t[0].numel() == G * co * Mp // e:
            gt = g_t[0]                           # written by the BatchNorm backward that produced g (vidc_bn_train_backward_t)
        else:
            if g is None:
                raise RuntimeError("wgrad %s: neither dY nor a matching dY^T" % (key,))
            gt = self._empty(G * co, Mp // e)
            L.check(lib.vidc_im2col_transposed(L.ptr(g), L.ptr(gt), B, Ho, Wo, G * co, _ld(g), Ho, Wo, 1, 1, 1, 0, Mp, split, st), "transpose dY")
        # rows of Xt in channel-major order (split + 4): the GEMM's output [co][ci*taps + tap] IS the OIHW weight gradient, written in place
        # (no staging buffer, no permute / copy launch)
        inplace = self.wgrad_inplace            # False: tap-major rows, staging buffer, permute / copy (A/B, tests)
        if bf16 and taps == 1 and stride == 1 and pad == 0 and x.bf is not None and self.xt_from_bf16:
            # 1x1 / stride 1: Xt is the plain transpose of x, taken from the bf16 operand copy the forward conv read (half the bytes, same bits)
            L.check(lib.vidc_transpose_bf16(L.ptr(x.bf), L.ptr(xt), M, G * ci, Mp, st), "transpose x (bf16)")
        elif bf16 and inplace and x.bf is not None and self.xt_from_bf16 and B * H * W * G * ci < (1 << 31):
            # any other geometry: the transposed im2col gathered from the bf16 copy as well (half the input bytes of the fp32 source)
            L.check(lib.vidc_im2col_transposed_bf16(L.ptr(x.bf), L.ptr(xt), B, H, W, G * ci, Ho, Wo, kh, kw, stride, pad, Mp, st), "im2col^T (bf16)")
        else:
            L.check(lib.vidc_im2col_transposed(L.ptr(x.t), L.ptr(xt), B, H, W, G * ci, x.ld, Ho, Wo, kh, kw, stride, pad, Mp, split | (4 if inplace else 0), st), "im2col^T")
        n_out = taps * ci
        gw = self._adjacent_base(self.grad, keys, ".weight")      # grouped: the G gradients are one contiguous run, group g at + g * co * n_out
        tmp = gw if inplace else self._empty(co, n_out)
        d = L.gemm_desc(co, Mp, n_out, groups=G, ldx=Mp, ldy=n_out, precision=self.precision, planar=G > 1, x=L.ptr(gt), w=L.ptr(xt), y=L.ptr(tmp),
                        scale1=L.ptr(self._const(self._ones, n_out, 1.0)), shift1=L.ptr(self._const(self._zeros, n_out, 0.0)))
        self._plan(d, "gemm")
        L.check(lib.vidc_conv2d_bn_act(C.byref(d), st), "wgrad gemm")
        if not inplace:
            if taps == 1:
                gw.view(co, ci).copy_(tmp)
            else:
                L.check(lib.vidc_wgrad_permute(L.ptr(tmp), L.ptr(gw), co, ci, taps, st), "wgrad permute")
        return True

    def conv(self, x, key, stride=1, pad=0, relu=False, out=None):
        """nn.Conv2d (+ReLU when no BatchNorm sits in between, depth_completion.py:141-142).  Records its backward."""
        keys = _keys(key)                        # G > 1: the same layer of the three pyramids as one grouped launch (x, y: G channel slices)
        G = len(keys)
        w = self.param[keys[0] + ".weight"]
        bias = self.param.get(keys[0] + ".bias")
        if G > 1 and bias is not None:
            raise RuntimeError("grouped conv %s: a bias per group is not supported (the pyramids' convs have none)" % (keys,))
        co, ci, kh, kw = w.shape
        B, H, W, cx = x.t.shape
        if cx != G * ci:
            raise RuntimeError("conv %s: input has %d channels, expected %d x %d" % (keys[0], cx, G, ci))
        Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        wp = self._pack(key, "f", w)
        if self.precision == L.PREC_BF16 and x.bf is None and ci % 64 == 0:      # the bf16 operand copy, made once per activation: every conv that
            x.bf = self._empty(B, H, W, G * ci // 2)                               # reads x uses it, and so does the weight-gradient transpose
            L.check(L.lib().vidc_cast_bf16(L.ptr(x.t), L.ptr(x.bf), B * H * W, G * ci, x.ld, L.current_stream()), "cast")
        y = Act(out if out is not None else self._empty(B, Ho, Wo, G * co))
        y.conv_out = not relu and self.dyt_fused
        # stride 1, no bias, bf16 operands, GEMM weight gradient: this conv's backward reads dY only as bf16 rows (dgrad) and as dY^T (wgrad)
        y.no_f32_grad = (y.conv_out and self.skip_f32_dy and self.precision == L.PREC_BF16 and stride == 1 and bias is None and co % 64 == 0 and
                         B * Ho * Wo < (1 << 31) and self._wgrad_fits((B, H, W, ci, Ho, Wo, co, kh, kw, stride, pad), G) and (G == 1 or self.wgrad_inplace))
        # (VIDC_TRAIN_CONV_STATS_MAX_M bounds the output rows it is used for: one partial per 32 rows makes the final reduction of a large
        #  map long -- 4800 partials at M = 153 600 -- but limiting it to 16 384 or 3 000 rows measured the same step time within 0.2 ms)
        if self.conv_stats and self.precision == L.PREC_BF16 and not relu and out is None and co % 32 == 0 and B * Ho * Wo <= self.conv_stats_max_m:
            y.stats = torch.empty(((B * Ho * Wo + 31) // 32) * 2 * G * co, dtype=torch.float64, device=self.device)
        self._conv_call(x.t, wp, bias if bias is not None else self._const(self._zeros, co, 0.0), y.t, kh, kw, stride, pad, relu, False, x_bf=x.bf, stats=y.stats,
                        groups=G)

        def backward():
            g, g_bf, g_t = y.grad, y.grad_bf, y.grad_t
            if g is None:
                # the BatchNorm backward skipped the fp32 dY (no_f32_grad): this closure must then find BOTH bf16 forms, in the geometry
                # its GEMMs expect -- anything else (a second consumer of y, a precision switched between forward and backward) would
                # read a stand-in tensor as if it were the gradient
                Mp_ = (B * Ho * Wo + 63) // 64 * 64
                if not (y.no_f32_grad and not relu and g_bf is not None and g_t is not None and self.precision == L.PREC_BF16 and
                        g_t[1] == Mp_ and g_t[0].numel() == G * co * Mp_ // 2):
                    raise RuntimeError("conv %s: no fp32 gradient and no matching bf16 forms of it (no_f32_grad invariant broken)" % (key,))
            if relu:                                         # y = relu(conv): mask first
                gm = self._empty(B, Ho, Wo, G * co)
                L.check(L.lib().vidc_relu_backward(L.ptr(g), L.ptr(y.t), L.ptr(gm), y.rows, G * co, _ld(g), y.ld, G * co, 0, L.current_stream()), "relu_bwd")
                g, g_bf, g_t = gm, None, None
            lib = L.lib()

            def weight_and_bias_gradient(g=g, g_t=g_t):     # (column sums for the bias); on the lane's side stream: see __init__
                if not self._wgrad_gemm(g, x, key, (B, H, W, ci, Ho, Wo, co, kh, kw, stride, pad), g_t=g_t):
                    if g is None:
                        raise RuntimeError("wgrad %s: the direct kernel needs the fp32 dY" % (key,))
                    for gi, k in enumerate(keys):                # (shapes beyond the GEMM's 32-bit limits: the direct kernel, group by group)
                        sc = self._scratch_bytes(lib.vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, co, ci, kh, kw))
                        L.check(lib.vidc_conv_wgrad(L.ptr(g[..., gi * co:(gi + 1) * co]), L.ptr(x.t[..., gi * ci:(gi + 1) * ci]), L.ptr(self.grad[k + ".weight"]), B, H, W,
                                                    ci, x.ld, Ho, Wo, co, _ld(g), kh, kw, stride, pad, L.ptr(sc), L.current_stream()), "wgrad")
                if bias is not None:
                    L.check(lib.vidc_colsum(L.ptr(g), y.rows, co, _ld(g), L.ptr(self.grad[keys[0] + ".bias"]), L.ptr(self._train_scratch(y.rows, co)),
                                            L.current_stream()), "colsum")

            self._beside(weight_and_bias_gradient)
            if x.grad is False:                              # network input: no data gradient wanted
                return
            # data gradient: the conv kernel on flipped / transposed weights; a strided conv spreads dY over the input grid first
            wd = self._pack(key, "d", w)
            gz = g
            if stride > 1:
                gz, g_bf = self._empty(B, H, W, G * co), None
                L.check(lib.vidc_zero_stuff(L.ptr(g), L.ptr(gz), B, Ho, Wo, G * co, _ld(g), stride, H, W, L.current_stream()), "zero_stuff")
            acc = x.grad is not None
            if not acc:
                x.grad = self._empty(B, H, W, G * ci)
            if acc:
                x.grad_bf = x.grad_t = None                  # x.grad changes below
            # (gz None: the BatchNorm backward wrote dY as bf16 only -- y.t stands in for its geometry, the kernel reads g_bf)
            self._conv_call(gz if gz is not None else y.t, wd, self._const(self._zeros, ci, 0.0), x.grad, kh, kw, 1, kh - 1 - pad, False, acc, x_bf=g_bf,
                            groups=G)

        self._record(backward)
        return y

    # ---- BatchNorm (train mode) + ReLU ---------------------------------------------------------------------------------------------
    def bn(self, x, key, relu, out=None, residual=None):
        """BatchNorm2d in train mode (+ReLU).  residual: the Bottleneck tail in the same pass, y = relu?(bn(x) + residual) -- the value and
        the backward are those of bn(x, relu=False) followed by add(., residual, relu); the add's launch and its pass over the map go."""
        Cc = x.t.shape[-1]
        keys = _keys(key)            # G > 1: ONE BatchNorm launch over the G x C channels of a grouped tensor; the G parameter / gradient /
        y = Act(out if out is not None else torch.empty_like(x.t))      # running-statistics vectors are contiguous runs of the flat buffers
        mean, rstd = self._empty(Cc), self._empty(Cc)
        gamma, beta = self._adjacent_base(self.param, keys, ".weight"), self._adjacent_base(self.param, keys, ".bias")
        if gamma.numel() * len(keys) != Cc:
            raise RuntimeError("bn %s: %d channels for %d x %d parameters" % (keys[0], Cc, len(keys), gamma.numel()))
        run_mean, run_var = self._adjacent_base(self.buf, keys, ".running_mean"), self._adjacent_base(self.buf, keys, ".running_var")
        g_gamma, g_beta = self._adjacent_base(self.grad, keys, ".weight"), self._adjacent_base(self.grad, keys, ".bias")
        bf16 = self.precision == L.PREC_BF16 and Cc % 64 == 0
        if bf16:
            y.bf = self._empty(*x.t.shape[:-1], Cc // 2)
        if x.stats is not None and x.stats.numel() == ((x.rows + 31) // 32) * 2 * Cc and x.ld == Cc:
            # x is a conv's output and the conv's epilogue has written its channel sums: final reduction + apply pass only
            L.check(L.lib().vidc_bn_train_forward_stats(L.ptr(x.t), L.ptr(y.t), x.rows, Cc, x.ld, y.ld, L.ptr(gamma), L.ptr(beta), L.ptr(run_mean),
                                                        L.ptr(run_var), BN_EPS, BN_MOMENTUM, int(relu), L.ptr(mean), L.ptr(rstd),
                                                        L.ptr(y.bf) if y.bf is not None else None, L.ptr(residual.t) if residual is not None else None,
                                                        residual.ld if residual is not None else 0, L.ptr(x.stats), L.ptr(self._train_scratch(x.rows, Cc)),
                                                        L.current_stream()), "bn_forward (conv stats)")
            x.stats = None                    # (consumed; the buffer goes back to the allocator with the activation's other temporaries)
        else:
            L.check(L.lib().vidc_bn_train_forward_add(L.ptr(x.t), L.ptr(y.t), x.rows, Cc, x.ld, y.ld, L.ptr(gamma), L.ptr(beta), L.ptr(run_mean),
                                                      L.ptr(run_var), BN_EPS, BN_MOMENTUM, int(relu), L.ptr(mean), L.ptr(rstd),
                                                      L.ptr(y.bf) if y.bf is not None else None, L.ptr(residual.t) if residual is not None else None,
                                                      residual.ld if residual is not None else 0, L.ptr(self._train_scratch(x.rows, Cc)), L.current_stream()), "bn_forward")
        self._nbt += [self.buf[k + ".num_batches_tracked"] for k in keys]
        y_in = y               # what the BatchNorm part of the backward takes dy from
        if residual is not None:
            y_in = Act(y.t)    # (geometry only: its .grad is the masked gradient handed on by the add part)

        def add_backward():    # the add's backward (training.add): mask by the ReLU, hand the gradient to both summands
            g = y.grad
            if relu:
                gm = self._empty(*y.t.shape)
                L.check(L.lib().vidc_relu_backward(L.ptr(g), L.ptr(y.t), L.ptr(gm), y.rows, Cc, _ld(g), y.ld, Cc, 0, L.current_stream()), "relu_bwd")
                g = gm
            y_in.grad = g
            self._accumulate(residual, g)

        mask_relu = relu and residual is None      # with a residual the ReLU sits behind the sum: its mask is applied by add_backward

        def backward():
            if residual is not None:
                add_backward()
            acc = x.grad is not None
            skip_f32 = (not acc) and bf16 and x.conv_out and x.no_f32_grad and x.rows < (1 << 31)      # dY is read through its two bf16 forms only
            dx = self._empty(*x.t.shape) if acc else None
            target = dx if acc else (None if skip_f32 else self._empty(*x.t.shape))
            tbf = self._empty(*x.t.shape[:-1], Cc // 2) if (bf16 and not acc) else None
            # x = a conv's output: dx is that conv's dY, and its weight-gradient GEMM wants dY^T as bf16 rows [C][Mp] -- written here, by the
            # kernel that produces dY, instead of by a transpose launch of its own (one launch and one pass over dY less per conv)
            Mp = (x.rows + 63) // 64 * 64
            tbt = self._empty(Cc, Mp // 2) if (tbf is not None and x.conv_out and x.rows < (1 << 31)) else None
            L.check(L.lib().vidc_bn_train_backward_t(L.ptr(y_in.grad), L.ptr(x.t), L.ptr(y.t) if mask_relu else None, L.ptr(target) if target is not None else None,
                                                     x.rows, Cc, _ld(y_in.grad), x.ld, y.ld,
                                                     Cc, L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(g_gamma), L.ptr(g_beta),
                                                     L.ptr(tbf) if tbf is not None else None, L.ptr(tbt) if tbt is not None else None, Mp,
                                                     L.ptr(self._train_scratch(x.rows, Cc)), L.current_stream()), "bn_backward")
            if acc:
                self._accumulate(x, target)
            else:
                x.grad, x.grad_bf, x.grad_t = target, tbf, ((tbt, Mp) if tbt is not None else None)

        self._record(backward)
        return y

    def flush_counters(self):
        """Every BatchNorm's num_batches_tracked += 1 for the forward just recorded, in one launch (bookkeeping, not arithmetic)."""
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)
        self._nbt = []

    def _accumulate(self, x, g):
        """x.grad += g (or = g when none yet; g is then shared, not copied: nothing writes it afterwards)."""
        if x.grad is None:
            x.grad = g
            return
        x.grad_bf = x.grad_t = None                          # the in-place sum below makes the bf16 copies of x.grad stale
        Cc = x.t.shape[-1]
        L.check(L.lib().vidc_relu_backward(L.ptr(g), None, L.ptr(x.grad), x.rows, Cc, _ld(g), 0, _ld(x.grad), 1, L.current_stream()), "accumulate")

    def add(self, a, b, relu, out=None):
        Cc = a.t.shape[-1]
        y = Act(out if out is not None else self._empty(*a.t.shape))
        if self.precision == L.PREC_BF16 and Cc % 64 == 0 and relu and self.add_bf16:      # a block output: the next block's convs read it as a bf16 operand
            y.bf = self._empty(*a.t.shape[:-1], Cc // 2)
        L.check(L.lib().vidc_add_rows_bf16(L.ptr(a.t), L.ptr(b.t), L.ptr(y.t), a.rows, Cc, a.ld, b.ld, y.ld, int(relu),
                                           L.ptr(y.bf) if y.bf is not None else None, L.current_stream()), "add")

        def backward():
            g = y.grad
            if relu:
                gm = self._empty(*a.t.shape)
                L.check(L.lib().vidc_relu_backward(L.ptr(g), L.ptr(y.t), L.ptr(gm), a.rows, Cc, _ld(g), y.ld, Cc, 0, L.current_stream()), "relu_bwd")
                g = gm
            self._accumulate(a, g)
            self._accumulate(b, g)

        self._record(backward)
        return y

    def maxpool(self, x):
        B, H, W, Cc = x.t.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = Act(self._empty(B, Ho, Wo, Cc))
        L.check(L.lib().vidc_maxpool3x3s2(L.ptr(x.t), L.ptr(y.t), B, H, W, Cc, x.ld, Cc, None, L.current_stream()), "maxpool")

        def backward():
            dx = self._empty(B, H, W, Cc)
            L.check(L.lib().vidc_maxpool3x3s2_backward(L.ptr(x.t), L.ptr(y.grad), L.ptr(dx), B, H, W, Cc, x.ld, _ld(y.grad), Cc, L.current_stream()), "maxpool_bwd")
            self._accumulate(x, dx)

        self._record(backward)
        return y

    def upsample(self, x, size):
        B, h, w, Cc = x.t.shape
        y = Act(self._empty(B, size[0], size[1], Cc))
        L.check(L.lib().vidc_upsample_bilinear_ac(L.ptr(x.t), L.ptr(y.t), B, h, w, Cc, x.ld, size[0], size[1], Cc, 0, None, L.current_stream()), "upsample")

        def backward():
            dx = self._empty(B, h, w, Cc)
            L.check(L.lib().vidc_upsample_bilinear_ac_backward(L.ptr(y.grad), L.ptr(dx), B, h, w, Cc, _ld(y.grad), Cc, size[0], size[1], L.current_stream()),
                    "upsample_bwd")
            self._accumulate(x, dx)

        self._record(backward)
        return y

    # ---- network walk (depth_completion.py:16-65, 154-165) ----------------------------------------------------------------------
    def _stem(self, x_nchw, p, out_channels=64):
        w = self.param[p + "conv1.conv1_1.weight"]
        B, cin, H, W = x_nchw.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = Act(self._empty(B, Ho, Wo, out_channels))
        L.check(L.lib().vidc_stem_conv3x3s2(L.ptr(x_nchw), L.ptr(w), L.ptr(y.t), B, cin, H, W, out_channels, out_channels, 1, None, 0, L.current_stream()), "stem")

        def backward():
            g = self._empty(B, Ho, Wo, out_channels)
            L.check(L.lib().vidc_relu_backward(L.ptr(y.grad), L.ptr(y.t), L.ptr(g), y.rows, out_channels, _ld(y.grad), out_channels, out_channels, 0,
                                               L.current_stream()), "relu_bwd")
            sc = self._scratch_bytes(L.lib().vidc_stem_wgrad_scratch_bytes(B, cin, H, W, out_channels))
            L.check(L.lib().vidc_stem_wgrad(L.ptr(g), L.ptr(x_nchw), L.ptr(self.grad[p + "conv1.conv1_1.weight"]), B, cin, H, W, out_channels, out_channels,
                                            L.ptr(sc), L.current_stream()), "stem_wgrad")

        self._record(backward)
        return y

    def _bottleneck(self, x, p, stride, project, out=None):
        """p: the block's parameter prefix, or one prefix per pyramid (grouped: x and the result hold the pyramids as channel slices)."""
        t = self.bn(self.conv(x, _cat(p, "conv1")), _cat(p, "bn1"), True)
        t = self.bn(self.conv(t, _cat(p, "conv2"), stride, 1), _cat(p, "bn2"), True)
        if not self.bn_add_fused:
            t = self.bn(self.conv(t, _cat(p, "conv3")), _cat(p, "bn3"), False)
            idn = self.bn(self.conv(x, _cat(p, "downsample.0"), stride, 0), _cat(p, "downsample.1"), False) if project else x
            return self.add(t, idn, True, out=out)
        t = self.conv(t, _cat(p, "conv3"))
        idn = self.bn(self.conv(x, _cat(p, "downsample.0"), stride, 0), _cat(p, "downsample.1"), False) if project else x
        return self.bn(t, _cat(p, "bn3"), True, out=out, residual=idn)      # relu(bn3(.) + identity) in the BatchNorm's apply pass

    def _stem_grouped(self, xs, ps, out_channels=64):
        """The three pyramids' stem convs (Cin 3, 3, 1: three small launches) into the channel slices of ONE [B, Ho, Wo, 3 x 64] tensor."""
        B, _c, H, W = xs[0].shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        G = len(ps)
        Ct = G * out_channels
        y = Act(self._empty(B, Ho, Wo, Ct))
        for g, (x_nchw, pp) in enumerate(zip(xs, ps)):
            L.check(L.lib().vidc_stem_conv3x3s2(L.ptr(x_nchw), L.ptr(self.param[pp + "conv1.conv1_1.weight"]), L.ptr(y.t[..., g * out_channels:]), B, x_nchw.shape[1],
                                                H, W, out_channels, Ct, 1, None, 0, L.current_stream()), "stem")

        def backward():
            g_ = self._empty(B, Ho, Wo, Ct)
            L.check(L.lib().vidc_relu_backward(L.ptr(y.grad), L.ptr(y.t), L.ptr(g_), y.rows, Ct, _ld(y.grad), Ct, Ct, 0, L.current_stream()), "relu_bwd")
            for g, (x_nchw, pp) in enumerate(zip(xs, ps)):
                cin = x_nchw.shape[1]
                sc = self._scratch_bytes(L.lib().vidc_stem_wgrad_scratch_bytes(B, cin, H, W, out_channels))
                L.check(L.lib().vidc_stem_wgrad(L.ptr(g_[..., g * out_channels:]), L.ptr(x_nchw), L.ptr(self.grad[pp + "conv1.conv1_1.weight"]), B, cin, H, W, out_channels,
                                                Ct, L.ptr(sc), L.current_stream()), "stem_wgrad")

        self._record(backward)
        return y

    def _pyramid(self, x_nchw, p, module, level_out):
        """ResNetPyramids.forward (depth_completion.py:55-65) in train mode; level l's output goes to `level_out[l]` (a channel slice of
        the concat buffer, depth_completion.py:151-152)."""
        grouped = not isinstance(p, str)      # p: one prefix per pyramid, x_nchw: their inputs; level_out[l]: the whole concat buffer of level l
        t = self._stem_grouped(x_nchw, p) if grouped else self._stem(x_nchw, p)
        t = self.bn(self.conv(t, _cat(p, "conv1.conv1_2"), 1, 1), _cat(p, "conv1.bn_2"), True)
        t = self.bn(self.conv(t, _cat(p, "conv1.conv1_3"), 1, 1), _cat(p, "conv1.bn1_3"), True)
        t = self.bn(t, _cat(p, "bn1"), True)
        t = self.maxpool(t)
        outs = []
        for li in range(1, 5):
            stage = getattr(module, "layer%d" % li)
            for bi, blk in enumerate(stage):
                last = bi == len(stage) - 1
                t = self._bottleneck(t, _cat(p, "layer%d.%d." % (li, bi)), blk.stride, blk.downsample is not None, out=level_out[li - 1] if last else None)
            outs.append(t)
        return outs

    def _decoder(self, levels, sizes, multi):
        """The four decoder branches by `_BRANCH_PLAN` (conv + BatchNorm + ReLU / upsample; widths from the parameters' shapes) and their sum
        z1 + z2 + z3 + z4.  The branches are independent until the sum: one stream lane each when `multi`."""
        main = torch.cuda.current_stream()

        def branch(b):
            t = levels[b - 1]
            idx, target = 0, b
            for step in _BRANCH_PLAN[b]:
                q = "feature%d_upsamping.%d" % (b, idx)
                if step == "u":
                    target -= 1
                    t = self.upsample(t, sizes[target - 1])
                    idx += 1
                else:
                    k = step[0]
                    t = self.bn(self.conv(t, q, 1, k // 2), "feature%d_upsamping.%d" % (b, idx + 1), True)
                    idx += 3
            return t

        zs = []
        for b in (1, 2, 3, 4):                       # the four decoder branches are independent until z1 + z2 + z3 + z4: one lane each
            if not multi:
                zs.append(branch(b))
                continue
            side = self._lane_streams()[b - 1]
            side.wait_stream(main)
            self._cur = b
            with torch.cuda.stream(side):
                zs.append(branch(b))
            self._cur = 0
        if multi:
            for side in self._lane_streams():
                main.wait_stream(side)
        return self.add(self.add(self.add(zs[0], zs[1], False), zs[2], False), zs[3], False)

    def head(self, h, key, pad, out_hw, relu):
        """The network's last op: the 1x1 conv `key` with padding `pad` and up to four output channels -> bilinear (align_corners) to out_hw ->
        ReLU if `relu`.  Returns the (B, Cout, H, W) planes as an Act; the backward turns their .grad into h.grad and the conv's gradients."""
        lib = L.lib()
        w2, b2 = self.param[key + ".weight"], self.param[key + ".bias"]
        co, ch = w2.shape[0], w2.shape[1]
        B, hh, hw_ = h.t.shape[:3]
        H, W = out_hw
        ph, pw = hh + 2 * pad, hw_ + 2 * pad
        low = self._empty(B, co, ph, pw)
        y = Act(self._empty(B, co, H, W))
        L.check(lib.vidc_head_conv1x1_upsample(L.ptr(h.t), L.ptr(w2), L.ptr(b2), L.ptr(low), L.ptr(y.t), B, hh, hw_, ch, h.ld, co, pad, H, W, int(relu),
                                               L.current_stream()), "head")

        def head_backward():
            g, n = y.grad, y.t.numel()
            if relu:
                g = self._empty(n)
                L.check(lib.vidc_relu_backward(L.ptr(y.grad), L.ptr(y.t), L.ptr(g), n // 4, 4, 4, 4, 4, 0, L.current_stream()), "relu_bwd")
            g_low = self._empty(B * co, ph, pw)                  # the planar gradient is B * Cout one-channel images
            L.check(lib.vidc_upsample_bilinear_ac_backward(L.ptr(g), L.ptr(g_low), B * co, ph, pw, 1, 1, 1, H, W, L.current_stream()), "upsample_bwd")
            h.grad = self._empty(B, hh, hw_, ch)
            sc = self._scratch_bytes(lib.vidc_head_backward_multi_scratch_bytes(B, hh, hw_, ch, co, pad))
            L.check(lib.vidc_head_backward_multi(L.ptr(g_low), L.ptr(h.t), L.ptr(w2), L.ptr(h.grad), L.ptr(self.grad[key + ".weight"]),
                                                 L.ptr(self.grad[key + ".bias"]), B, hh, hw_, ch, h.ld, ch, co, pad, L.ptr(sc), L.current_stream()), "head_bwd")

        self._record(head_backward)
        return y

    @staticmethod
    def _level_sizes(H, W):
        """(h, w) of the four pyramid levels of an H x W image: the stem and the max-pool halve it, then each of three stages does."""
        def half(s):
            return (s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1
        sizes = [half(half((H, W)))]
        for _ in range(3):
            sizes.append(half(sizes[-1]))
        return sizes

    def _begin_forward(self):
        self.tape, self._nbt = [], []
        self.repack()

    def _end_forward(self, pred):
        """pred: the Act of the network's output; the loss writes pred.grad, which the tape starts from."""
        self._pred = pred
        self.flush_counters()
        return pred.t

    def _run_tape(self, stop_after_decoder=False):
        """Runs the recorded backward closures, last first, each on the stream lane it was recorded on.  stop_after_decoder: return once
        the decoder's part is done (its last closure hands the level gradients to the pyramids), leaving the pyramids' closures in
        self.tape for a second call -- the caller starts the all-reduce of the decoder's gradients in between."""
        # Lifetime of cross-lane tensors: a closure owns the last references to activations / gradients that OTHER lanes still read or
        # write (levels[l].grad is allocated by a decoder branch on lane 1 and its channel slices are accumulated into by the pyramids on
        # lanes 2 and 3).  Dropping a closure right after it ran would hand such a block back to the allocating lane's pool while the
        # other lanes' kernels are still queued -- and inside a captured graph, where the three pyramids are parallel branches and a
        # freed block is reusable at once, the allocating lane's next temporary could overwrite it.  So every closure that has run is
        # kept until all lanes have joined the main stream at the end of the tape.  Cost: the backward's peak memory is the SUM of the
        # activation gradients and their bf16 / transposed forms instead of the live set (not measured; bounded by the gradient volume of
        # one backward, i.e. of the order of the forward's activations -- a few GB at batch 8, 320x240, of 288 GB);
        # a step that raises drops them at once (the except below), so a failed step does not pin them until the next good one.
        try:
            self._run_tape_inner(stop_after_decoder)
        except BaseException:
            self.tape, self._keepalive = [], []           # a failed step must not pin every activation gradient until the next good one
            raise

    def _run_tape_inner(self, stop_after_decoder):
        main = torch.cuda.current_stream()
        forked = []
        while self.tape:
            fn = self.tape.pop()
            self._keepalive.append(fn)
            lane = getattr(fn, "_lane", 0)
            if lane == 0 or self.n_lanes <= 1:
                for side in forked:
                    main.wait_stream(side)
                forked = []
                fn()
                if stop_after_decoder and getattr(fn, "_decoder_done", False):
                    self._join_wgrad(main)                # the decoder's weight gradients are complete before their all-reduce starts
                    return                                # (closures stay parked: the second call releases them after its join)
                continue
            side = self._lane_streams()[lane - 1]
            if side not in forked:
                side.wait_stream(main)                    # the work recorded before this lane's (decoder backward / loss) is on main
                forked.append(side)
            self._cur = lane
            with torch.cuda.stream(side):
                fn()
            self._cur = 0
        for side in forked:
            main.wait_stream(side)
        self._join_wgrad(main)
        self._keepalive = []                              # every lane has joined: nothing queued anywhere still touches these tensors

    @torch.no_grad()
    def optimizer_step(self, reduced=False):
        """torch.optim.Adam.step over the flat buffers; gradients are summed over ranks first (frame-sharded batch) unless `step` has
        done that already, overlapped with the backward.

        With an optimizer option set or an accumulation window open (class docstring) the order is: g += the window's sum, ONE all-reduce of
        that sum, the norm pass (when max_grad_norm is not None), then `vidc_optimizer_step`; otherwise `vidc_adam_step`, as ever."""
        lib, n, st = L.lib(), self.flat_p.numel(), L.current_stream()
        window = self._window
        if window:
            if reduced:
                raise RuntimeError("optimizer_step(reduced=True) with an accumulation window open: the gradient must be all-reduced after the window's sum is added")
            L.check(lib.vidc_grad_accumulate(L.ptr(self.flat_acc), L.ptr(self.flat_g), n, 2, st), "accumulate")
            self._window = 0
        if not reduced:
            self.buckets.all_reduce(self.flat_g)
        self.step_count += 1
        if not self._options_on and not window:
            L.check(lib.vidc_adam_step(L.ptr(self.flat_p), L.ptr(self.flat_g), L.ptr(self.m), L.ptr(self.v), n, self.lr, self.betas[0],
                                       self.betas[1], self.eps, self.step_count, st), "adam")
        else:
            grad_scale = 1.0 / (window + 1) if self.accumulate_mean else 1.0
            nseg, begin, begin_host, lr_scale, decay, flags = self._seg if self._seg is not None else (0, None, None, None, None, None)
            if self._norm_record is not None:      # (the norm needs the table only for its frozen flags)
                L.check(lib.vidc_grad_sqnorm(L.ptr(self.flat_g), n, nseg if self._any_frozen else 0, L.ptr(begin), begin_host, L.ptr(flags), grad_scale, self.max_grad_norm,
                                             L.ptr(self._norm_record), L.ptr(self._norm_scratch), st), "grad norm")
            L.check(lib.vidc_optimizer_step(L.ptr(self.flat_p), L.ptr(self.flat_g), L.ptr(self.m), L.ptr(self.v), n, self.lr, self.betas[0], self.betas[1],
                                            self.eps, self.step_count, int(self.decoupled_weight_decay), L.ptr(self._norm_record), grad_scale, nseg, L.ptr(begin),
                                            begin_host, L.ptr(lr_scale), L.ptr(decay), L.ptr(flags), st), "optimizer")
        self._packed_fresh = False      # so are the trainer's own packed copies (re-made by the next forward's repack())
        self.cnn._invalidate()          # the inference programs' packed / BN-folded copies are stale now

    def _distributed(self):
        from .sharding import collectives_active
        return collectives_active()

    cut_at_decoder = False      # across ranks, cut the backward where the decoder's part ends and all-reduce its gradients under the rest

    def _check_inputs(self, tensors):
        """What a step refuses, before any capture starts."""
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("%s takes GPU tensors only (no CPU fallback)" % type(self).__name__)
        if not self.cnn.training:
            raise RuntimeError("call cnn.train() first (network_run.py:232): the trainer implements BatchNorm's train() mode")

    def _after_step(self):
        """Hook: what a subclass keeps of the step that just ran."""

    @torch.no_grad()
    def _forward_backward(self, ins, multi=False):
        """(loss, pred) of `forward` on the first three inputs and `loss_and_backward` on the rest; multi: the tape stops after the decoder."""
        self._check_inputs(ins)
        pred = self.forward(*ins[:3])
        if multi:
            return self.loss_and_backward(pred, *ins[3:], stop_after_decoder=True), pred
        return self.loss_and_backward(pred, *ins[3:]), pred

    def _reduce_around(self, rest):
        """Multi-rank: starts the all-reduce of the decoder's gradients, runs `rest` (the pyramids' backward) under it, then starts the others'."""
        waits = self.buckets.all_reduce_async(self.flat_g, self._dec_off, None)
        rest()
        return waits + self.buckets.all_reduce_async(self.flat_g, 0, self._dec_off)

    def _eager_forward_backward(self, ins, multi):
        loss, _ = self._forward_backward(ins, multi)
        return loss, (self._reduce_around(self._run_tape) if multi else [])

    def _graphed(self, ins, multi=False):
        """A step's forward + backward on `ins`: eager the first two times a shape is seen (that creates the packed-weight table, constants,
        scratch and split-K workspaces), then captured once (`_forward_backward` on static copies of the inputs) and replayed.  Returns
        (loss, completion callbacks of the all-reduces started)."""
        key = tuple((tuple(t.shape), t.dtype) for t in ins) + (multi,)
        ent = self._graphs.get(key)
        if ent is None:
            seen = self._graph_seen[key] = self._graph_seen.get(key, 0) + 1
            if seen <= 2:                     # eager: creates the packed-weight table, constants, scratch and split-K workspace
                return self._eager_forward_backward(ins, multi)
            static = [t.clone() for t in ins]
            torch.cuda.synchronize()
            graph, rest = torch.cuda.CUDAGraph(), None
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):      # (RCCL's watchdog thread polls events while this thread captures)
                loss, pred = self._forward_backward(static, multi)
            if multi:                         # second graph: the pyramids' backward (same memory pool: it reads the first one's tensors)
                rest = torch.cuda.CUDAGraph()
                with torch.cuda.graph(rest, pool=graph.pool(), capture_error_mode="thread_local"):
                    self._run_tape()
            ent = self._graphs[key] = (graph, rest, static, loss, pred)
        graph, rest, static, loss, pred = ent
        for dst, src in zip(static, ins):
            dst.copy_(src)
        self._packed_fresh = True             # the graph starts with repack()
        graph.replay()
        return loss.clone(), (self._reduce_around(rest.replay) if rest is not None else [])

    def step(self, *ins):
        """One `_run_training_iteration` on the subclass's inputs (`forward`'s three, then the loss's): returns the loss (0-dim fp64 GPU
        tensor, this rank's frames).

        The forward + backward of a step is ~4000 launches from Python (~17 us of host time each: host-bound once the convs run in the
        bf16 modes), all with shape-static arguments, so from the third step of a given input shape on it is replayed as captured
        hipGraphs (VIDC_TRAIN_GRAPH=0: always eager).  The all-reduce and the Adam launch (its bias correction takes the step number
        by value) stay outside the graphs.  Across ranks the depth trainer's backward is cut where the decoder's part ends
        (`cut_at_decoder`): the all-reduce of the decoder's gradients (59 % of the 1.24 GB) is started there and runs under the pyramids'
        backward, the rest follows.  A step that closes an accumulation window (`backward_only`) takes the uncut path: the decoder's early
        all-reduce would run before the window's sum exists, so `optimizer_step` adds the sum and all-reduces it once."""
        multi = self.cut_at_decoder and self._distributed() and not self._window
        self._check_bindings()
        self._check_inputs(ins)
        loss, waits = self._graphed(ins, multi) if self.use_graph else self._eager_forward_backward(ins, multi)
        for w in waits:
            w()
        self.optimizer_step(reduced=multi)
        self.last_loss = loss
        self._after_step()
        return loss

    def backward_only(self, *ins):
        """A micro-step of an accumulation window: the forward + backward of `step` on `ins` (captured / replayed like a step's; BatchNorm's
        running statistics move as in any train-mode forward), then the gradient is added to the window's sum `flat_acc` (allocated on first
        use; fp32 adds, outside the graphs like the Adam launch).  No all-reduce, no optimizer launch.  Returns the loss.  The next `step`
        closes the window."""
        self._check_bindings()
        self._check_inputs(ins)
        loss, _ = self._graphed(ins, False) if self.use_graph else self._eager_forward_backward(ins, False)
        if self.flat_acc is None:
            self.flat_acc = torch.empty_like(self.flat_g)
        L.check(L.lib().vidc_grad_accumulate(L.ptr(self.flat_acc), L.ptr(self.flat_g), self.flat_g.numel(), 1 if self._window else 0, L.current_stream()),
                "accumulate")
        self._window += 1
        self.last_loss = loss
        self._after_step()
        return loss


class DepthCompletionTrainer(_TrainerBase):
    """`_run_training_iteration` of `ModifiedFPN` (module docstring): three ResNet-101 pyramids (`self.layout`: "grouped" = interleaved per parameter
    name, the multi-rank default; "per_pyramid" otherwise), the 192-wide decoder, the padded one-channel head, the masked L1 depth loss."""

    cut_at_decoder = True

    def forward(self, image, normal, depth_in):
        """Train-mode forward; returns the predicted depth (B,1,H,W).  The tape of backward closures is left in self.tape."""
        self._begin_forward()
        B, _, H, W = image.shape
        sizes = self._level_sizes(H, W)
        chans = [256, 512, 1024, 2048]
        cat = [self._empty(B, sizes[l][0], sizes[l][1], 3 * chans[l]) for l in range(4)]
        levels = [Act(c) for c in cat]
        subs = []
        # The three pyramids are independent until the decoder: each runs on its own HIP stream (forward here, backward in
        # loss_and_backward), so the fixed cost of one pyramid's ~100 small launches hides under the other two's -- in the captured graph
        # they are three parallel branches.  Scratch and split-K workspaces are per lane.  VIDC_TRAIN_STREAMS=1: one stream.
        main = torch.cuda.current_stream()
        multi = self.n_lanes > 1
        if self.grouped:
            # ONE chain of grouped launches for the three pyramids on the caller's stream: a third of the launches, each three times the
            # work; level l's last block writes the concat buffer directly and the decoder reads the very same activation object, so the
            # decoder's d(concat) IS the pyramids' level gradient (no slicing step)
            xs = [t.contiguous().float() for t in (image, normal, depth_in)]
            levels = self._pyramid(xs, tuple(n + "." for n in PYRAMIDS), getattr(self.cnn, PYRAMIDS[0]), cat)
        for pi, (name, x) in enumerate(() if self.grouped else (("resnet_rgb", image), ("resnet_normal", normal), ("resnet_depth", depth_in))):
            outs = [cat[l][..., pi * chans[l]:(pi + 1) * chans[l]] for l in range(4)]
            x = x.contiguous().float()
            if not multi:
                subs.append(self._pyramid(x, name + ".", getattr(self.cnn, name), outs))
                continue
            side = self._lane_streams()[pi]
            side.wait_stream(main)
            self._cur = pi + 1
            with torch.cuda.stream(side):
                subs.append(self._pyramid(x, name + ".", getattr(self.cnn, name), outs))
            self._cur = 0
        if multi and not self.grouped:
            for side in self._lane_streams():
                main.wait_stream(side)

        def split_level_grads():                     # runs (in the backward) once the decoder has produced d(concat): slices become the
            for l in range(4 if not self.grouped else 0):      # gradients of the three pyramids' level outputs (grouped: the same objects)
                for pi in range(3):
                    g = levels[l].grad[..., pi * chans[l]:(pi + 1) * chans[l]]
                    subs[pi][l].grad = g if subs[pi][l].grad is None else subs[pi][l].grad
        # NB: appended BEFORE the decoder ops, so it runs after all of them in the reversed tape; a level's slice is also fed by the next
        # stage of its pyramid, whose backward (later in the reversed order) accumulates into the same slice.
        split_level_grads._decoder_done = True       # everything recorded after this point (= run before it) is the decoder's backward
        self._record(split_level_grads)

        z = self._decoder(levels, sizes, multi)
        h = self.conv(z, "feature_concat.0", 1, 1, relu=True)
        # padded 1x1 head -> bilinear to (H, W) -> ReLU (depth_completion.py:143-147)
        return self._end_forward(self.head(h, "feature_concat.2", 1, (H, W), relu=True))

    def loss_and_backward(self, pred, depth_gt, stop_after_decoder=False):
        """network_run.py:163-173 + `total_loss.backward()`: fills the flat gradient buffer; returns the loss (0-dim fp64 GPU tensor)."""
        B, _, H, W = pred.shape
        n = pred.numel()
        gt = depth_gt.contiguous().float()
        loss = torch.zeros((), dtype=torch.float64, device=self.device)
        dpred = self._pred.grad = self._empty(n)
        terms = self._empty(n)
        sc = self._scratch_bytes((n // 512 + 64) * 8)
        L.check(L.lib().vidc_masked_l1_loss(L.ptr(pred), L.ptr(gt), n, H * W, L.ptr(loss), L.ptr(dpred), L.ptr(terms), L.ptr(sc), L.current_stream()),
                "loss")
        self._run_tape(stop_after_decoder)
        return loss

    def forward_backward(self, image, normal, depth_in, depth_gt):
        return self._forward_backward((image, normal, depth_in, depth_gt))

    def step(self, image, normal, depth_in, depth_gt):
        return super().step(image, normal, depth_in, depth_gt)


class SurfaceNormalTrainer(_TrainerBase):
    """`_run_training_iteration` (network_run.py:231-254) for `self.cnn = SurfaceNormalPrediction`, i.e. a `DefaultImageNetwork(...,
    estimates_normal=True)` run: `SurfaceNormalTrainer(cnn, learning_rate).step(image, gravity, alignment, normal_gt, mask)`.

        cnn.train(); normals = cnn(image, gravity, alignment)      surface_normal.py:147-171: forward warp, the ResNet-101 pyramid, the four
                                                                   128-wide decoder branches, feature_concat, inverse warp + R^T + F.normalize
        loss, angle = compute_normal_vectors_loss_l1(F.normalize(normal_gt), normals, mask > 0)      network_run.py:181-189
        loss.backward(); Adam(cnn.parameters(), lr).step()

    normalize_prediction is the loss's own argument (normal_utils.py:20).  True, its default, calls `Normalize`, a name the reference never
    defines; it is read as F.normalize(., dim=1, eps=1e-12) (include/vidc.h, vidc_normal_l1_loss).  False is the reference's code as shipped.
    No gradient is taken with respect to the image: neither the forward warp's adjoint nor the stem's data gradient runs.  `last_angle`
    is the reference's `other_outputs['angle']` before rounding (a 0-dim fp64 GPU tensor), `last_count` the N the loss was divided by.

    Refused: `use_mask=True` networks (the masked branch needs a mask-multiply backward) and a process group of more than one rank -- N
    is a per-batch count here, so the sum of the ranks' gradients is not the reference's gradient (the depth loss divides by the
    constant H*W, which is why that step shards)."""

    pyramid_names = ("resnet_pyramids",)

    def __init__(self, cnn, learning_rate=1e-4, betas=(0.9, 0.999), eps=1e-8, normalize_prediction=True, **optimizer_options):
        """optimizer_options: weight_decay, decoupled_weight_decay, max_grad_norm, param_groups, accumulate_mean (`_TrainerBase`)."""
        if getattr(cnn, "use_mask", False):
            raise RuntimeError("SurfaceNormalTrainer: use_mask=True networks are not supported (surface_normal.py:150-162 multiplies the features by the "
                               "warp's validity mask; that multiply has no backward here yet)")
        self._refuse_ranks()
        super().__init__(cnn, learning_rate, betas, eps, **optimizer_options)
        self.normalize_prediction = bool(normalize_prediction)
        self._stats = torch.zeros(3, dtype=torch.float64, device=self.device)      # loss, N, angle sum of the step that ran last (written by the loss kernel)
        self.last_angle = self.last_count = None

    def _check_inputs(self, tensors):
        self._refuse_ranks()
        super()._check_inputs(tensors)

    def _refuse_ranks(self):
        if self._distributed():
            raise RuntimeError("SurfaceNormalTrainer runs on one rank only: the normal loss divides by N, the number of unmasked pixels of the batch "
                               "(normal_utils.py:32-33), so gradients summed over ranks that each divide by their own N are not the reference's gradient")

    def forward(self, image, gravity, alignment):
        """Train-mode forward of surface_normal.py:147-171; returns the unit normals (B,3,H,W).  The tape of backward closures is left in self.tape."""
        wp = self.cnn.warp_2dof_alignment
        B, cin, H, W = image.shape
        if (H, W) != (wp.H, wp.W) or tuple(self.cnn.output_size) != (H, W) or cin != 3:
            raise RuntimeError("SurfaceNormalTrainer: the network is built for 3 x %d x %d images (cc_img) and output_size %s, got %d x %d x %d"
                               % (wp.H, wp.W, tuple(self.cnn.output_size), cin, H, W))
        self._begin_forward()
        lib, ac = L.lib(), int(wp.align_corners)
        g = gravity.reshape(B, 3).contiguous().float()
        a = alignment.reshape(B, 3).contiguous().float()
        params = self._empty(B, L.WARP_PARAMS)
        L.check(lib.vidc_warp2dof_params(L.ptr(g), L.ptr(a), B, wp.fx, wp.fy, wp.cx, wp.cy, L.ptr(wp.kinv(self.device)), W, H, L.ptr(params), L.current_stream()),
                "warp params")
        x = image.contiguous().float()
        warped = torch.empty_like(x)
        L.check(lib.vidc_warp2dof_fwd(L.ptr(x), L.ptr(params), L.ptr(warped), B, 3, H, W, wp.cx, wp.cy, ac, L.current_stream()), "warp")
        # one pyramid on the caller's stream; the decoder's branches read its level outputs directly, so their d(level) accumulates into the
        # activation the next stage's backward adds to
        levels = self._pyramid(warped, "resnet_pyramids.", self.cnn.resnet_pyramids, [None] * 4)
        z = self._decoder(levels, self._level_sizes(H, W), self.n_lanes > 1)
        h = self.conv(z, "feature_concat.0", 1, 1, relu=True)
        # unpadded three-channel 1x1 head -> bilinear to (H, W) (surface_normal.py:143-144) -> inverse warp + R^T + F.normalize (:166-170)
        raw = self.head(h, "feature_concat.2", 0, (H, W), relu=False)
        pred = Act(self._empty(B, 3, H, W))
        L.check(lib.vidc_warp2dof_inv_rot_norm(L.ptr(raw.t), L.ptr(params), L.ptr(pred.t), B, H, W, wp.cx, wp.cy, ac, 1, L.current_stream()), "inverse warp")

        def inverse_warp_backward():
            raw.grad = self._empty(B, 3, H, W)
            L.check(lib.vidc_warp2dof_inv_rot_norm_backward(L.ptr(raw.t), L.ptr(pred.grad), L.ptr(params), L.ptr(raw.grad), B, H, W, wp.cx, wp.cy, ac, 1,
                                                            L.current_stream()), "inverse warp_bwd")

        self._record(inverse_warp_backward)
        return self._end_forward(pred)

    def loss_and_backward(self, pred, normal_gt, mask):
        """network_run.py:181-189 + `total_loss.backward()`: fills the flat gradient buffer; returns the loss (0-dim fp64 GPU tensor).  The
        angle sum and N of this step are in `self._stats` ([loss, N, angle])."""
        B, _, H, W = pred.shape
        gt = normal_gt.contiguous().float()
        m = mask.reshape(B, H, W).contiguous().float()
        if tuple(gt.shape) != (B, 3, H, W):
            raise RuntimeError("SurfaceNormalTrainer: normal_gt must be (B, 3, H, W) = %s, got %s" % ((B, 3, H, W), tuple(gt.shape)))
        dpred = self._pred.grad = self._empty(B, 3, H, W)
        st = self._stats
        sc = self._scratch_bytes(L.lib().vidc_normal_l1_loss_scratch_bytes(B, H, W))
        L.check(L.lib().vidc_normal_l1_loss(L.ptr(pred), L.ptr(gt), L.ptr(m), B, H, W, int(self.normalize_prediction), L.ptr(st), L.ptr(st[1:]), L.ptr(st[2:]),
                                            L.ptr(dpred), L.ptr(sc), L.current_stream()), "normal loss")
        self._run_tape()
        return st[0].clone()

    def forward_backward(self, image, gravity, alignment, normal_gt, mask):
        return self._forward_backward((image, gravity, alignment, normal_gt, mask))

    def step(self, image, gravity, alignment, normal_gt, mask):
        """`_TrainerBase.step`; `last_angle` holds the step's angle sum and `last_count` its N."""
        return super().step(image, gravity, alignment, normal_gt, mask)

    def _after_step(self):
        self.last_count, self.last_angle = self._stats[1].clone(), self._stats[2].clone()
