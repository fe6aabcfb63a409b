"""Host side of the HIP engine: records a network as a `Program` (array of C launch descriptors over
device buffers), plans buffers, folds BatchNorm, packs weights, and runs the whole thing through ONE
C-ABI call per frame (`vidc_program_run` / hipGraph replay).  PyTorch is used for device memory and
streams only; there is no eager or CPU execution path here.

Layout: activations are NHWC fp32.  A "grouped" tensor (G > 1) keeps the G groups as channel slices of
one [B,H,W,G*C] buffer, so the rgb/normal/depth pyramids of ModifiedFPN run as one grouped launch per
layer and `torch.cat((rgb, normal, depth), dim=1)` (depth_completion.py:151-152) costs nothing.
"""
import collections
import ctypes as C
import json
import os

import torch

from . import _lib as L


class K(tuple):
    """Tuple of parameter-name prefixes (one per group); `K + 'conv1'` appends to every member."""

    def __new__(cls, items):
        return super().__new__(cls, (items,) if isinstance(items, str) else tuple(items))

    def __add__(self, s):
        return K(p + s for p in self)


def _keys(k):
    return k if isinstance(k, K) else K(k)


class T:
    """Program tensor: NHWC view (channel slice) of a planned buffer; NCHW for program inputs/outputs."""
    __slots__ = ("buf", "B", "H", "W", "C", "G", "ld", "ch_off", "nchw", "esz")

    def __init__(self, buf, B, H, W, Cc, G=1, ld=None, ch_off=0, nchw=False, esz=4):
        self.buf, self.B, self.H, self.W, self.C, self.G = buf, B, H, W, Cc, G
        self.ld = ld if ld is not None else G * Cc
        self.ch_off, self.nchw = ch_off, nchw
        self.esz = esz           # bytes per channel: 4, or 2 for a plain-bf16 image (Program.cast), whose ld / ch_off count bf16 channels

    @property
    def numel(self):
        return self.B * self.H * self.W * self.ld


class WeightStore:
    """Device-resident derived parameters of one nn.Module: packed conv weights and folded BN affines.
    Rebuilt lazily after `invalidate()` (load_state_dict / .cuda() / .to())."""

    def __init__(self, module):
        self.module = module
        self._cache = {}
        self._sd = None
        self._virtual = {}       # name -> fn(state_dict) : derived entries (e.g. a Linear weight re-laid-out for NHWC activations)
        self.bn_eps = 1e-5       # nn.BatchNorm2d's default; 0 for the detector's FrozenBatchNorm2d (layers/batch_norm.py: no eps)

    def add_virtual(self, name, fn):
        if name not in self._virtual:
            self._virtual[name] = fn
            self._sd = None

    def invalidate(self):
        self._cache.clear()
        self._sd = None

    def sd(self):
        if self._sd is None:
            self._sd = {k: v.detach() for k, v in self.module.state_dict().items()}
            for name, fn in self._virtual.items():
                self._sd[name] = fn(self._sd)
        return self._sd

    def raw(self, key):
        return self.sd()[key]

    def packed(self, keys, dry_run=False, precision=0):
        """The weights of the G groups `keys` packed by the C kernels for FORMATS[precision], in float32-typed storage [G][Cout][welems]:
        [KH][KW][Cin] fp32, the split-bf16 image of the same bytes, K bf16 values (64 channels per K unit), or the K * 33 / 32 bytes of
        the MXFP8 images (include/vidc.h)."""
        ck = ("w", precision) + tuple(keys)
        if ck not in self._cache:
            ws = [self.sd()[k + ".weight"].contiguous() for k in keys]
            co, ci, kh, kw = ws[0].shape
            fmt = FORMATS[precision]
            out = torch.empty((len(ws), co, fmt.welems(kh * kw * ci)), dtype=torch.float32, device=ws[0].device)
            for g, w in enumerate(ws):
                assert tuple(w.shape) == (co, ci, kh, kw)
                if not dry_run:
                    L.check(getattr(L.lib(), fmt.pack)(L.ptr(w), L.ptr(out[g]), co, ci, kh, kw, L.current_stream()), "pack")
            if dry_run:
                return out
            self._cache[ck] = out
        return self._cache[ck]

    def packed_winograd(self, keys, m, dry_run=False, precision=0):
        """U = G g G^T of the 3x3 filters `keys` for F(m x m, 3x3): [G][(m+2)^2][Cout][Cin] fp32 (csrc/winograd.hip, fp64 inside), or the
        split-bf16 image of the same bytes (precision 1) -- the weights of the (m+2)^2 * G group 1x1 GEMM launch."""
        ck = ("wino", m, precision) + tuple(keys)
        if ck not in self._cache:
            ws = [self.sd()[k + ".weight"].contiguous() for k in keys]
            co, ci, kh, kw = ws[0].shape
            assert (kh, kw) == (3, 3)
            a2 = (m + 2) * (m + 2)
            out = torch.empty((len(ws) * a2, co, ci), dtype=torch.float32, device=ws[0].device)
            if dry_run:
                return out
            for g, w in enumerate(ws):
                assert tuple(w.shape) == (co, ci, 3, 3)
                L.check(L.lib().vidc_winograd_weight_transform(L.ptr(w), L.ptr(out[g * a2]), co, ci, m, L.current_stream()), "winograd weights")
            if precision == L.PREC_BF16X3:
                img = torch.empty_like(out)
                L.check(L.lib().vidc_pack_conv_weight_bf16x3(L.ptr(out), L.ptr(img), len(ws) * a2 * co, ci, 1, 1, L.current_stream()), "pack")
                out = img
            self._cache[ck] = out
        return self._cache[ck]

    def packed_winograd_fused(self, keys, dry_run=False):
        """U of F(4 x 4, 3x3) in the fragment order of the one-launch kernel (vidc_winograd_weight_pack_fused): 36 Cout Cin floats per group."""
        ck = ("winof",) + tuple(keys)
        if ck not in self._cache:
            u = self.packed_winograd(keys, 4, dry_run, 0)
            out = torch.empty_like(u)
            if dry_run:
                return out
            co, ci = u.shape[1], u.shape[2]
            for g in range(len(keys)):
                L.check(L.lib().vidc_winograd_weight_pack_fused(L.ptr(u[g * 36]), L.ptr(out[g * 36]), co, ci, L.current_stream()), "winograd weights (fused order)")
            self._cache[ck] = out
        return self._cache[ck]

    def identity_affine(self, co, device):
        ck = ("id", co, str(device))
        if ck not in self._cache:
            self._cache[ck] = (torch.ones(co, dtype=torch.float32, device=device), torch.zeros(co, dtype=torch.float32, device=device))
        return self._cache[ck]

    def affine(self, conv_keys, bn_keys):
        """Per-output-channel (scale, shift) [G][Cout] for conv(+bias) followed by eval-mode BN, folded in fp64."""
        ck = ("a",) + tuple(conv_keys) + tuple(bn_keys or ())
        if ck not in self._cache:
            sd = self.sd()
            scales, shifts = [], []
            for g, ckey in enumerate(conv_keys):
                co = sd[ckey + ".weight"].shape[0] if ckey is not None else sd[bn_keys[g] + ".weight"].shape[0]
                dev = sd[(ckey or bn_keys[g]) + ".weight"].device
                bias = sd.get(ckey + ".bias") if ckey is not None else None
                bias = bias.double() if bias is not None else torch.zeros(co, dtype=torch.float64, device=dev)
                if bn_keys is not None:
                    bn = bn_keys[g]
                    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + self.bn_eps)
                    t = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s + bias * s
                else:
                    s, t = torch.ones(co, dtype=torch.float64, device=dev), bias
                scales.append(s.float())
                shifts.append(t.float())
            self._cache[ck] = (torch.stack(scales).contiguous(), torch.stack(shifts).contiguous())
        return self._cache[ck]


class JointWeightStore(WeightStore):
    """Derived parameters of several modules behind one key space: key "name/param" resolves to `modules[name]`'s
    state_dict entry "param".  Lets one Program (one grouped launch per layer) span networks -- the software-pipelined
    frame program of pipeline.InterleavedPrograms runs the surface-normal pyramid of frame i+1 and the three
    depth-completion pyramids of frame i as four groups of the same launches."""

    def __init__(self, modules):
        super().__init__(None)
        self.modules = dict(modules)

    def sd(self):
        if self._sd is None:
            self._sd = {"%s/%s" % (name, k): v.detach() for name, m in self.modules.items() for k, v in m.state_dict().items()}
            for name, fn in self._virtual.items():
                self._sd[name] = fn(self._sd)
        return self._sd


_TUNING = None


def tuning_table():
    """Optional per-shape (tile, splitk) overrides measured on MI355X (tools/autotune.py writes it)."""
    global _TUNING
    if _TUNING is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_tuning.json")
        _TUNING = json.load(open(path)) if os.path.exists(path) else {}
        if os.environ.get("VIDC_TUNING_OVERRIDE"):          # experiment knob: '{"M80_N256_K256_k1s1_G144": [40, 64]}' replaces / adds entries (A-B runs of one signature)
            _TUNING = dict(_TUNING)
            _TUNING.update(json.loads(os.environ["VIDC_TUNING_OVERRIDE"]))
    return _TUNING


def precision_mode():
    """VIDC_PRECISION=fp32  : every conv on fp32 MFMA (exact fp32; the reference mode).
       VIDC_PRECISION=mixed : (default) compute-bound convs run split-bf16 3-pass MFMA (per-shape choice from the measured
                              table, else by size); whole-path depth RMSE vs fp32 ~1.4e-5, bar 1e-3.
       VIDC_PRECISION=mxfp8 : the direct convs that mxfp8_layer() selects run block-scaled FP8 (VIDC_PREC_MXFP8, include/vidc.h);
                              every other layer makes exactly the choice of the mixed mode.
       VIDC_PRECISION=bf16  : the direct convs that bf16_layer() selects run on plain bf16 operands with fp32 accumulation (VIDC_PREC_BF16:
                              one MFMA pass and half the operand bytes of the mixed mode's split bf16); every other layer makes exactly
                              the choice of the mixed mode.  Opt-in."""
    return os.environ.get("VIDC_PRECISION", "mixed")


def default_precision(flops):
    return L.PREC_BF16X3 if flops >= 1.5e9 else L.PREC_FP32


MXFP8_MIN_FLOPS = 1e8       # below this a layer is launch-bound: the FP8 rate buys nothing and the quantisation costs a launch
# layers kept out of MXFP8 for accuracy (key substrings; DESIGN 4.6 lists the sets measured): ResNet-101 layer 1 and the FPN decoders
# with the convs in front of the heads -- the pyramid's layers 2-4 run in MXFP8
MXFP8_EXCLUDED = ("layer1.", "_upsamping.", "feature_concat.")


def mxfp8_layer(key, co, ci, flops):
    """Whether the direct conv `key` runs in MXFP8 in the mxfp8 mode: 128-channel K units (Cin % 128), whole 32-channel output tiles,
    enough work (FLOPs of the launch, all groups), and not one of the layers MXFP8_EXCLUDED keeps out for accuracy."""
    return ci % 128 == 0 and co % 32 == 0 and flops >= MXFP8_MIN_FLOPS and not any(e in key for e in MXFP8_EXCLUDED)


# layers kept out of plain bf16 for accuracy (key substrings, as MXFP8_EXCLUDED): none -- every qualifying layer runs in bf16
BF16_EXCLUDED = ()


def bf16_layer(key, co, ci, flops):
    """Whether the direct conv `key` runs in plain bf16 in the bf16 mode: whole 64-channel K units (128 bytes of a bf16 row), whole
    32-channel output tiles, and not one of the layers BF16_EXCLUDED keeps out.  No size threshold: a small layer between two bf16
    layers would otherwise cost its producer an fp32 store and itself a split launch."""
    return ci % 64 == 0 and co % 32 == 0 and not any(e in key for e in BF16_EXCLUDED)


def winograd_mode():
    """VIDC_WINOGRAD=auto : (default) 3x3 / stride 1 / pad 1 convs with >= 128 input channels run as Winograd F(m x m, 3x3) GEMMs
                             (csrc/winograd.hip): the entry "W:<direct signature>" of the measured table picks m in {0, 2, 4} (5 = m 4 in ONE launch, fp32 only), else (fp32 mode
                             only) m = 4 on maps of at least 24 rows and columns and m = 2 below; the mixed mode without a table entry stays direct.
       VIDC_WINOGRAD=0 / 2 / 4 : never / always that m where the layer qualifies (tests, A/B runs)."""
    return os.environ.get("VIDC_WINOGRAD", "auto")


def winograd_choice(B, H, W, co, ci, kh, kw, stride, padding, dilation, G, mode=None, precision=None, reduced=False):
    """reduced: the caller runs this layer in a reduced-precision operand format (Program.conv: MXFP8 by mxfp8_layer, plain bf16 by
    bf16_layer): no Winograd -- the transforms amplify the rounding of the operands, and the direct form is what the FP8 / bf16 rate
    pays for.  Every other layer of the mxfp8 and bf16 modes takes the mixed mode's choice."""
    if reduced or (kh, kw, stride, padding, dilation) != (3, 3, 1, 1, 1) or ci % 32 or co % 32:
        return 0
    mode = mode if mode is not None else winograd_mode()
    precision = precision if precision is not None else precision_mode()
    if precision in ("mxfp8", "bf16"):
        precision = "mixed"
    if mode in ("0", "2", "4"):
        m = int(mode)
    else:
        ent = None                                # [m in the fp32 mode, m in the mixed mode]; measured on the frame program (4 pyramid groups):
        for gg in (G, 4, 3, 1, 2):                # the stand-alone programs run the same layers with 1 / 3 groups and take that verdict
            ent = tuning_table().get("W:" + conv_signature(L.conv_desc(B, H, W, ci, co, 3, 3, 1, 1, groups=gg)))
            if ent is not None:
                break
        if ent is not None:
            m = int(ent[1 if precision == "mixed" else 0]) if isinstance(ent, (list, tuple)) else int(ent)
            if m == 5 and gg != G:                 # 5 = F(4 x 4) in ONE launch (csrc/wfused.hip): measured for exactly that group count
                m = 4
        elif ci < 128 or precision == "mixed":
            # no measured verdict for this shape.  fp32: the heuristic below.  mixed: the direct form -- in the committed table the bf16x3
            # direct conv beats the transform + GEMM + transform triple for 73 of 112 layers (three launches and two HBM round trips through
            # V and M against a conv that is cheap already), so an untuned resolution or batch must not default to the slower form
            m = 0
        else:
            m = 4 if min(H, W) >= 24 else 2
    if m:
        mt = 4 if m == 5 else m
        a2 = (mt + 2) * (mt + 2)
        tiles = B * (-(-H // mt)) * (-(-W // mt))
        if tiles * a2 * G * max(ci, co) * 4 >= 2 ** 31 or B * (-(-H // mt)) > 65535:     # 32-bit buffer offsets in the GEMM kernel / grid.y
            return 0
    return m


def conv_signature(d):
    """Key of a launch in the measured tables (conv_tuning.json, train_tuning.json): GEMM rows, Cout, K, kernel height, stride and
    groups of its descriptor -- L.conv_desc / L.gemm_desc without pointers give the key of a launch before it is built."""
    return "M%d_N%d_K%d_k%ds%d_G%d" % (d.B * d.Ho * d.Wo, d.Cout, d.KH * d.KW * d.Cin, d.KH, d.stride, d.groups)


# One row per conv operand format (VIDC_PREC_* of include/vidc.h); everything this file knows about a format is in its row.
#   name, pack, welems: the display name; the C entry point that packs a weight; the float32-typed elements of one packed group of
#                       K = KH * KW * Cin values.
# The activation side of the three reduced formats -- the image of an fp32 tensor that such a conv reads (Program.image):
#   kind, op          : the recorded op that makes the image, and its vidc_op_kind
#   unit              : channels of a K unit; a row of an image holds whole units
#   esz               : bytes per channel of the image's T, whose ld / ch_off count such channels
#   elems             : float32-typed buffer elements of the image of `rows` pixels of `c` channels in `g` groups
#   sliceable         : a channel slice of an image, at a multiple of `unit`, is the image of that slice
#   folded            : the groups are channel slices of one row of C * G channels; otherwise every group is a plane pair of its own
#   out_flag, out_key : the conv flag that makes a producer's epilogue write the image, and the recorded key of that image
#   out_gs, out_esz   : in a conv descriptor d with out_flag, the elements from one group's image to the next, and the bytes of one
Format = collections.namedtuple("Format", "name pack welems kind op unit esz elems sliceable folded out_flag out_key out_gs out_esz",
                                defaults=(None,) * 11)
FORMATS = {
    L.PREC_FP32: Format("fp32", "vidc_pack_conv_weight", lambda k: k),
    L.PREC_BF16X3: Format("bf16x3", "vidc_pack_conv_weight_bf16x3", lambda k: k,          # a unit is [32 x hi | 32 x lo]: the 128 bytes of 32 floats
                          kind="split", op=L.OP_SPLIT, unit=32, esz=4, elems=lambda rows, c, g: rows * c * g, sliceable=True, folded=True,
                          out_flag=L.SPLIT_OUT, out_key="split_out", out_gs=lambda d: d.y_gs, out_esz=4),
    L.PREC_MXFP8: Format("mxfp8", "vidc_pack_conv_weight_mxfp8", lambda k: k // 128 * 33,  # per group a plane of e4m3 bytes, then its scales: 33 bytes per 32
                         kind="quant", op=L.OP_QUANT, unit=128, esz=4, elems=lambda rows, c, g: -(-g * rows * c * 33 // 128), sliceable=False,
                         folded=False, out_flag=L.MXFP8_OUT, out_key="mx_out", out_gs=lambda d: d.B * d.Ho * d.Wo * d.Cout * 33 // 128, out_esz=4),
    L.PREC_BF16: Format("bf16", "vidc_pack_conv_weight_bf16", lambda k: k // 2,            # dense rows of bf16 values: 64 channels are 128 bytes
                        kind="cast", op=L.OP_CAST, unit=64, esz=2, elems=lambda rows, c, g: rows * c * g // 2, sliceable=True, folded=True,
                        out_flag=L.BF16_OUT, out_key="bf16_out", out_gs=lambda d: d.y_gs, out_esz=2),
}
IMAGE_FORMATS = {f.kind: f for f in FORMATS.values() if f.kind}      # in the order Program._fuse_images folds them: split, quant, cast
OP_KINDS = dict({"conv": L.OP_CONV, "stem": L.OP_STEM, "maxpool": L.OP_MAXPOOL, "upsample": L.OP_UPSAMPLE, "head": L.OP_HEAD,
                 "warp_params": L.OP_WARP_PARAMS, "warp_fwd": L.OP_WARP_FWD, "warp_inv": L.OP_WARP_INV, "avgpool": L.OP_AVGPOOL,
                 "normalize": L.OP_NORMALIZE, "det_im2col": L.OP_DET_IM2COL, "mask": L.OP_MASK, "wino_in": L.OP_WINO_IN,
                 "wino_out": L.OP_WINO_OUT, "nearest2x": L.OP_NEAREST2X, "copy": L.OP_COPY}, **{f.kind: f.op for f in IMAGE_FORMATS.values()})
# precision mode -> (the direct convs it takes out of the mixed mode's choice, the format they run in)
MODE_LAYERS = {"mxfp8": (mxfp8_layer, L.PREC_MXFP8), "bf16": (bf16_layer, L.PREC_BF16)}


class Program:
    """Records ops symbolically (buffers are integers), then `finalize()` plans memory and builds the C program."""

    def __init__(self, weights, device, batch, reuse_buffers=True, mode=None, winograd=None):
        """mode: "fp32" | "mixed" | "mxfp8" | "bf16" (default: precision_mode()); winograd: "0" | "2" | "4" | "auto" (default: winograd_mode()) -- a program whose
        results feed DECISIONS (the plane-mask detector: score / IoU / mask thresholds) is recorded with mode="fp32", winograd="0": exact
        fp32 direct-form sums, the arithmetic its oracle pins."""
        self.ws, self.device, self.B = weights, device, batch
        self.ops = []            # (kind, dict)
        self.buf_elems = []      # elements per buffer id
        self.pinned = set()      # buffer ids that must not alias (inputs / outputs)
        self.inputs, self.outputs = {}, {}
        self.reuse = reuse_buffers and os.environ.get("VIDC_NO_BUFFER_REUSE", "0") != "1"      # (debug knob of tools/dbg_lanes.py: every program tensor in storage of its own)
        self.stream_id = 0
        self.wait_mask = 0
        self.handle = None
        self.flops = 0           # executed conv FLOPs (2*M*N*K summed; Winograd layers count their transform-domain GEMMs)
        self.direct_flops = 0    # the executed layers in direct form (what self.flops was before the Winograd layers)
        self.ref_flops = 0       # the same layers in the reference's formulation (1x1 convs AFTER their upsample: SURVEY §8d)
        self._keep = []
        self._images = {}        # (buf, precision, ch_off, channels of a row, planes) -> the image (T) of that fp32 tensor in FORMATS[precision]
        self.cuts = []           # op indices where a new segment starts (see cut()); filled by finalize()
        self._cut_markers = []
        self.n_fused_splits = self.n_fused_quants = self.n_fused_casts = self.n_fused_warps = 0      # image / warp ops folded by finalize()
        self.mode = mode if mode is not None else precision_mode()
        if self.mode not in ("fp32", "mixed", "mxfp8", "bf16"):
            raise ValueError("unknown precision mode %r (VIDC_PRECISION: fp32, mixed, mxfp8 or bf16)" % (self.mode,))
        self.winograd = winograd

    # ---- buffers ----------------------------------------------------------------------------------------
    def _new_buf(self, elems, pinned=False):
        self.buf_elems.append(int(elems))
        if pinned:
            self.pinned.add(len(self.buf_elems) - 1)
        return len(self.buf_elems) - 1

    def input_nchw(self, name, Cc, H, W):
        t = T(self._new_buf(self.B * Cc * H * W, True), self.B, H, W, Cc, nchw=True)
        self.inputs[name] = t
        return t

    def input_raw(self, name, elems):
        t = T(self._new_buf(elems, True), 1, 1, 1, elems)
        self.inputs[name] = t
        return t

    def mark_output(self, name, t):
        self.pinned.add(t.buf)
        self.outputs[name] = t

    def nhwc(self, H, W, Cc, G=1):
        return T(self._new_buf(self.B * H * W * G * Cc), self.B, H, W, Cc, G)

    def cut(self):
        """Starts a new segment: the ops recorded so far and the ops that follow can be captured / launched separately
        (capture_segments / launch_segment), with host-enqueued work in between."""
        assert self.ops, "cut() before the first op"
        self._cut_markers.append(self.ops[-1])      # identity of the last op of the segment (op indices shift in _fuse_images)

    def on_stream(self, sid, wait_mask=0):
        self.stream_id, self.wait_mask = sid, wait_mask

    def _written(self, t):
        """t's buffer is (re)written: its split / MXFP8 / bf16 images are stale."""
        self._images = {k: v for k, v in self._images.items() if k[0] != t.buf}

    def _emit(self, kind, reads, writes, **kw):
        kw.update(stream_id=self.stream_id, wait_mask=self.wait_mask)
        self.wait_mask = 0
        self.ops.append((kind, [t.buf for t in reads if t is not None], [t.buf for t in writes], kw))

    # ---- ops ---------------------------------------------------------------------------------------------
    def conv(self, x, key, bn=None, relu=False, stride=1, padding=0, bn2=None, relu2=False, residual=None,
             relu_after_residual=False, out=None, accumulate=False, ref_flops_scale=1.0, dilation=1):
        keys = _keys(key)
        G = len(keys)
        assert x.G == G and not x.nchw
        w0 = self.ws.raw(keys[0] + ".weight")
        co, ci, kh, kw = w0.shape
        assert ci == x.C, "conv %s expects Cin=%d, got %d" % (keys[0], ci, x.C)
        Ho = (x.H + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
        Wo = (x.W + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
        y = out if out is not None else self.nhwc(Ho, Wo, co, G)
        assert (y.H, y.W, y.C, y.G) == (Ho, Wo, co, G)
        self._written(y)     # y is (re)written
        flags = (L.RELU1 if relu else 0) | (L.AFFINE2 if bn2 is not None else 0) | (L.RELU2 if relu2 else 0)
        if residual is not None:
            assert (residual.H, residual.W, residual.C, residual.G) == (Ho, Wo, co, G)
            flags |= L.RESIDUAL | (L.RELU3 if relu_after_residual else 0)
        if accumulate:
            flags |= L.ACCUM
        flops = 2 * self.B * Ho * Wo * co * ci * kh * kw * G
        selects, reduced_prec = MODE_LAYERS.get(self.mode, (None, None))
        reduced = selects is not None and selects(keys[0], co, ci, flops)
        wm = 0
        if residual is None and not accumulate:
            wm = winograd_choice(self.B, x.H, x.W, co, ci, kh, kw, stride, padding, dilation, G, mode=self.winograd, precision=self.mode, reduced=reduced)
        if wm:
            self.ref_flops += int(round(flops * ref_flops_scale))
            self.direct_flops += flops
            # F(4 x 4) in ONE launch (csrc/wfused.hip): where the measured table says 5, or -- VIDC_WINO_FUSED=<tiles>, A-B runs -- every fp32
            # F(4 x 4) layer of at most that many tiles and VIDC_WINO_FUSED_MAXC (256) input channels; VIDC_WINO_FUSED=0 keeps the three launches everywhere
            knob = os.environ.get("VIDC_WINO_FUSED")
            fusable = self.mode == "fp32" and ci % 16 == 0 and not (flags & ~(L.RELU1 | L.AFFINE2 | L.RELU2))
            forced = (wm in (4, 5) and knob is not None and int(knob) > 0 and self.B * (-(-Ho // 4)) * (-(-Wo // 4)) <= int(knob)
                      and ci <= int(os.environ.get("VIDC_WINO_FUSED_MAXC", "256")))
            if fusable and (forced or (wm == 5 and knob is None)):
                return self._conv_winograd_fused(x, y, keys, bn, bn2, flags, (co, ci, Ho, Wo))
            return self._conv_winograd(x, y, keys, bn, bn2, flags, 4 if wm == 5 else wm, (co, ci, Ho, Wo))
        self.flops += flops
        self.direct_flops += flops
        self.ref_flops += int(round(flops * ref_flops_scale))
        sig = conv_signature(L.conv_desc(self.B, x.H, x.W, ci, co, kh, kw, stride, padding, dilation, G))
        prec = reduced_prec if reduced else self._table_precision(sig, flops)
        xin = self.image(x, prec) if FORMATS[prec].kind else x
        self._emit("conv", [xin, residual, y if accumulate else None], [y], x=xin, y=y, keys=keys, precision=prec,
                   bn=_keys(bn) if bn is not None else None, bn2=_keys(bn2) if bn2 is not None else None,
                   residual=residual, flags=flags, stride=stride, pad=padding, geom=(co, ci, kh, kw, Ho, Wo), dilation=dilation, sig=sig)
        return y

    def _conv_winograd(self, x, y, keys, bn, bn2, flags, m, geom):
        """3x3 / stride 1 / pad 1 conv + BN + ReLU as Winograd F(m x m, 3x3): input transform -> ONE grouped 1x1 GEMM launch with
        (m+2)^2 * G groups on the MFMA kernel -> output transform with the conv's epilogue (csrc/winograd.hip)."""
        co, ci, Ho, Wo = geom
        G = len(keys)
        a2 = (m + 2) * (m + 2)
        tiles = self.B * (-(-Ho // m)) * (-(-Wo // m))
        gflops = 2 * tiles * a2 * G * co * ci
        self.flops += gflops
        sig = conv_signature(L.gemm_desc(tiles, ci, co, groups=a2 * G))
        prec = self._table_precision(sig, gflops)
        V = T(self._new_buf(tiles * a2 * G * ci), 1, 1, tiles, ci, a2 * G)
        Mm = T(self._new_buf(tiles * a2 * G * co), 1, 1, tiles, co, a2 * G)
        self._emit("wino_in", [x], [V], x=x, v=V, m=m, cin=ci, split=int(prec == L.PREC_BF16X3))
        self._emit("conv", [V], [Mm], x=V, y=Mm, keys=keys, precision=prec, bn=None, bn2=None, residual=None, flags=0, stride=1, pad=0,
                   geom=(co, ci, 1, 1, 1, tiles), dilation=1, wino=m, sig=sig)
        self._emit("wino_out", [Mm], [y], mm=Mm, y=y, keys=keys, bn=_keys(bn) if bn is not None else None,
                   bn2=_keys(bn2) if bn2 is not None else None, flags=flags, m=m, cout=co)
        return y

    def _conv_winograd_fused(self, x, y, keys, bn, bn2, flags, geom):
        """The same layer as ONE launch (csrc/wfused.hip, tile VIDC_TILE_WINO4_FUSED): fp32, F(4 x 4), no V / M buffers.  Only behind VIDC_WINO_FUSED
        (measured equal to the three launches alone)."""
        co, ci, Ho, Wo = geom
        tiles = self.B * (-(-Ho // 4)) * (-(-Wo // 4))
        self.flops += 2 * tiles * 36 * len(keys) * co * ci
        self._emit("conv", [x], [y], x=x, y=y, keys=keys, precision=L.PREC_FP32, bn=_keys(bn) if bn is not None else None,
                   bn2=_keys(bn2) if bn2 is not None else None, residual=None, flags=flags, stride=1, pad=1, geom=(co, ci, 3, 3, Ho, Wo), dilation=1,
                   wino_fused=tiles, sig=conv_signature(L.gemm_desc(tiles, ci, co, groups=36 * len(keys))))      # (named by the products it executes)
        return y

    def _table_precision(self, sig, flops):
        """The operand format of a launch that the mode does not select itself (MODE_LAYERS): the entry of the measured table for its
        signature if there is one, else by size -- in every mode but fp32."""
        if self.mode == "fp32":
            return L.PREC_FP32
        ent = tuning_table().get(sig)
        return ent[2] if (ent is not None and len(ent) > 2) else default_precision(flops)

    def image(self, x, precision):
        """The image of the fp32 activation tensor x in the operand format FORMATS[precision] -- split bf16, MXFP8 or plain bf16 -- made
        once per tensor, by a launch of its own that finalize() folds into the producer of x where it can (_fuse_images).  Returns the
        caller's view of it: a T of the format's esz whose ld / ch_off count channels of the image."""
        fmt = FORMATS[precision]
        ch, planes = (x.C * x.G, 1) if fmt.folded else (x.C, x.G)       # (grouped and channel-concatenated views share one folded image)
        ck = (x.buf, precision, x.ch_off, ch, planes)
        if ck not in self._images:
            assert not x.nchw and x.esz == 4 and ch % fmt.unit == 0
            if fmt.sliceable:
                # a channel slice of a tensor whose image exists is a slice of that image: the layout keeps every unit (128 bytes) in
                # place, so only ch_off (a multiple of the unit) moves
                for (b0, p0, off0, ch0, _), img in self._images.items():
                    if (b0, p0) == (x.buf, precision) and off0 <= x.ch_off and x.ch_off + ch <= off0 + ch0 and (x.ch_off - off0) % fmt.unit == 0:
                        return T(img.buf, x.B, x.H, x.W, x.C, x.G, ld=img.ld, ch_off=x.ch_off - off0, esz=fmt.esz)
            y = T(self._new_buf(fmt.elems(x.B * x.H * x.W, x.C, x.G)), x.B, x.H, x.W, x.C, x.G, ld=ch, esz=fmt.esz)
            self._emit(fmt.kind, [x], [y], x=x, y=y)
            self._images[ck] = y
        return T(self._images[ck].buf, x.B, x.H, x.W, x.C, x.G, ld=ch, esz=fmt.esz)

    def split(self, x):
        return self.image(x, L.PREC_BF16X3)

    def quant(self, x):
        return self.image(x, L.PREC_MXFP8)

    def cast(self, x):
        return self.image(x, L.PREC_BF16)

    def level_image(self, t):
        """ONE image of a pyramid level for the decoders of this mode, which read channel slices of it: split bf16 in the mixed and mxfp8
        modes (written by the producing conv's epilogue; a split launch behind an MXFP8 producer), plain bf16 in the bf16 mode where the
        level has whole units (the producing conv's VIDC_BF16_OUT), none in fp32."""
        if self.mode == "bf16":
            if (t.C * t.G) % FORMATS[L.PREC_BF16].unit == 0:
                self.image(t, L.PREC_BF16)
        elif self.mode != "fp32":
            self.image(t, L.PREC_BF16X3)

    def linear(self, x, key, relu=False):
        """nn.Linear on `x.view(B, -1)` of the reference's NCHW tensor (surface_normal_dorn.py:23-24), as a 1x1 conv over the
        NHWC buffer viewed as one pixel with H*W*C channels; the weight columns are re-ordered (c,h,w) -> (h,w,c) once."""
        assert x.G == 1 and x.ld == x.C and x.ch_off == 0 and not x.nchw
        Cc, Hh, Ww = x.C, x.H, x.W
        vkey = "%s@hwc%dx%dx%d" % (key, Hh, Ww, Cc)

        def relayout(sd, key=key):
            w = sd[key + ".weight"]
            return w.view(w.shape[0], Cc, Hh, Ww).permute(0, 2, 3, 1).reshape(w.shape[0], Hh * Ww * Cc, 1, 1).contiguous()

        self.ws.add_virtual(vkey + ".weight", relayout)
        self.ws.add_virtual(vkey + ".bias", lambda sd, key=key: sd[key + ".bias"])
        flat = T(x.buf, x.B, 1, 1, Hh * Ww * Cc)
        return self.conv(flat, vkey, relu=relu)

    def avgpool(self, x, kernel, stride, padding):
        kh, kw = kernel
        sh, sw = stride
        ph, pw = padding
        Ho, Wo = (x.H + 2 * ph - kh) // sh + 1, (x.W + 2 * pw - kw) // sw + 1
        y = self.nhwc(Ho, Wo, x.C, x.G)
        self._emit("avgpool", [x], [y], x=x, y=y, geom=(kh, kw, sh, sw, ph, pw))
        return y

    def normalize_nchw(self, x):
        assert x.nchw
        y = T(self._new_buf(x.B * x.C * x.H * x.W), x.B, x.H, x.W, x.C, nchw=True)
        self._emit("normalize", [x], [y], x=x, y=y)
        return y

    def stem_conv(self, xs, key, relu=True, x_is_nchw=True):
        """xs: one NCHW tensor or a list (one per group, Cin may differ: 3,3,1)."""
        keys = _keys(key)
        xs = xs if isinstance(xs, (list, tuple)) else [xs]
        G = len(keys)
        assert len(xs) == G and x_is_nchw
        co = self.ws.raw(keys[0] + ".weight").shape[0]
        H, W = xs[0].H, xs[0].W
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        y = self.nhwc(Ho, Wo, co, G)
        for g in range(G):
            self._emit("stem", [xs[g]], [y], x=xs[g], y=y, key=keys[g], g=g, relu=relu)
        return y

    def det_im2col(self, image, Hp, Wp, mean_bgr):
        """The detector's input transform fused with the im2col of its 7x7/s2 stem (vidc_det_stem_im2col): image NCHW in [0,1] ->
        NHWC (B, Hp/2, Wp/2, 160)."""
        assert image.nchw and image.C == 3
        y = self.nhwc(Hp // 2, Wp // 2, 160)
        self._emit("det_im2col", [image], [y], x=image, y=y, geom=(image.H, image.W, Hp, Wp), mean=tuple(float(v) for v in mean_bgr))
        return y

    def nearest2x(self, x):
        y = self.nhwc(2 * x.H, 2 * x.W, x.C, x.G)
        self._emit("nearest2x", [x], [y], x=x, y=y)
        return y

    def mask_scale(self, x, image):
        """x * (r+g+b > 1e-2 of `image`, nearest-resized to x): the use_mask branch of surface_normal.py:150-162.  `image`: NCHW."""
        assert image.nchw and image.C == 3 and not x.nchw
        y = self.nhwc(x.H, x.W, x.C, x.G)
        self._emit("mask", [x, image], [y], x=x, y=y, image=image)
        return y

    def maxpool(self, x):
        Ho, Wo = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
        y = self.nhwc(Ho, Wo, x.C, x.G)
        self._emit("maxpool", [x], [y], x=x, y=y)
        return y

    def upsample(self, x, size, relu=False, into=None, out=None, sum_groups=False):
        """UpsamplingBilinear2d(size).  `into`: accumulate (+=) into an existing tensor; `out`: write (=) into an existing tensor
        (e.g. a channel slice of a concat buffer) instead of a new one.  sum_groups: x is a grouped tensor whose G upsampled (ReLU'd)
        groups are added up, group 0 first -- z2 + z3 + z4 of the decoders in one launch."""
        if sum_groups:
            assert into is not None and x.G > 1 and (into.H, into.W, into.C * into.G) == (size[0], size[1], x.C)
            self._written(into)
            self._emit("upsample", [x, into], [into], x=x, y=into, flags=(L.UP_RELU if relu else 0) | L.UP_ACCUM | (x.G << 8), sum_groups=x.G)
            return into
        y = into if into is not None else (out if out is not None else self.nhwc(size[0], size[1], x.C, x.G))
        assert (y.H, y.W, y.C * y.G) == (size[0], size[1], x.C * x.G)
        flags = (L.UP_RELU if relu else 0) | (L.UP_ACCUM if into is not None else 0)
        self._written(y)
        self._emit("upsample", [x, into], [y], x=x, y=y, flags=flags)
        return y

    def head(self, x, key, pad, out_size, relu):
        """1x1 conv to <=4 channels (+pad) -> upsample to out_size -> [relu]; returns the NCHW output tensor."""
        w = self.ws.raw(key + ".weight")
        co, ci = w.shape[0], w.shape[1]
        assert ci == x.C * x.G
        hp, wp = x.H + 2 * pad, x.W + 2 * pad
        low = T(self._new_buf(self.B * co * hp * wp), self.B, hp, wp, co, nchw=True)
        y = T(self._new_buf(self.B * co * out_size[0] * out_size[1]), self.B, out_size[0], out_size[1], co, nchw=True)
        self._emit("head", [x], [low, y], x=x, low=low, y=y, key=key, pad=pad, relu=relu)
        return y, low

    def warp_params(self, g, a, intr, kinv):
        p = T(self._new_buf(self.B * L.WARP_PARAMS), 1, 1, 1, self.B * L.WARP_PARAMS)
        self._emit("warp_params", [g, a, kinv], [p], g=g, a=a, kinv=kinv, p=p, intr=intr)
        return p

    def warp_fwd(self, x, params, intr, align_corners):
        y = T(self._new_buf(x.B * x.C * x.H * x.W), x.B, x.H, x.W, x.C, nchw=True)
        self._emit("warp_fwd", [x, params], [y], x=x, p=params, y=y, intr=intr, ac=int(align_corners))
        return y

    def warp_inv(self, x, params, intr, align_corners, normalize=True, out=None):
        """`out`: an existing NCHW (B,3,H,W) tensor to write into (e.g. the input buffer a later tick reads the normals from)."""
        y = out if out is not None else T(self._new_buf(x.B * 3 * x.H * x.W), x.B, x.H, x.W, 3, nchw=True)
        assert y.nchw and (y.B, y.C, y.H, y.W) == (x.B, 3, x.H, x.W)
        self._emit("warp_inv", [x, params], [y], x=x, p=params, y=y, intr=intr, ac=int(align_corners), norm=int(normalize))
        return y

    def copy(self, src, dst):
        self._emit("copy", [src], [dst], src=src, dst=dst)

    # ---- planning ----------------------------------------------------------------------------------------
    def _last_writer(self, i, buf):
        return next((t for t in range(i - 1, -1, -1) if buf in self.ops[t][2]), None)

    def _cut_between(self, marks, j, i):
        """A segment boundary between op j and op i (marks: the ids of the cut markers): what a fold moves from i to j must not depend on
        which segments ran."""
        return any(id(self.ops[t]) in marks for t in range(j, i))

    def _attach(self, t, fmt, img):
        """Op t writes `img`, the image of its result in the format fmt, as well."""
        kind, _r, writes, kw = self.ops[t]
        kw[fmt.out_key] = img
        if kind in ("conv", "wino_out"):
            kw["flags"] |= fmt.out_flag
        writes.append(img.buf)

    def _fold_split(self, i, kw, marks):
        """A split whose input was just produced by fused convs, max-pool, upsample or Winograd output kernels (VIDC_SPLIT_OUT / the y_split
        argument of the glue kernels) or by the stem launches of a grouped stem output.  Not behind a conv of another reduced format,
        which writes its own image."""
        fmt, xs = IMAGE_FORMATS["split"], kw["x"]
        j = self._last_writer(i, xs.buf)
        if j is None or self.ops[j][0] not in ("conv", "maxpool", "upsample", "stem", "wino_out"):
            return False
        if self.ops[j][0] == "stem":
            # G launches write the channel slices of one tensor: all of them get the image of the whole tensor
            y = self.ops[j][3]["y"]
            writers = [t for t in range(j + 1) if self.ops[t][0] == "stem" and self.ops[t][3]["y"].buf == y.buf]
            if xs.ch_off != 0 or xs.C * xs.G != y.C * y.G or y.ld != y.C * y.G or y.ld % fmt.unit or y.C % fmt.unit or \
                    any(self.ops[t][3].get(fmt.out_key) is not None for t in writers) or len(writers) != y.G:
                return False
            for t in writers:
                self._attach(t, fmt, kw["y"])
            return True
        # general case: the tensor is written by one producer, or slice by slice by several (a concat buffer filled by a conv and
        # an upsample, say); every producer writes its slice of the split image.  The slices must tile the split's channel range.
        last = {}                                        # channel slice -> its LAST writer (earlier ones are superseded)
        foreign = False
        for t in range(i):
            if xs.buf in self.ops[t][2]:
                if self.ops[t][0] not in ("conv", "maxpool", "upsample", "wino_out"):
                    foreign = True
                    continue
                yt = self.ops[t][3]["y"]
                if yt.buf == xs.buf:
                    last[(yt.ch_off, yt.C * yt.G)] = t
        writers = sorted(last.values())
        lo, hi = xs.ch_off, xs.ch_off + xs.C * xs.G
        ok = bool(writers) and not foreign and xs.ld % fmt.unit == 0 and lo % fmt.unit == 0
        cover = []
        for t in writers:
            yt, pk = self.ops[t][3]["y"], self.ops[t][3]
            ok = ok and yt.ld == xs.ld and yt.ch_off % fmt.unit == 0 and (yt.C * yt.G) % fmt.unit == 0 and lo <= yt.ch_off and \
                yt.ch_off + yt.C * yt.G <= hi and pk.get(fmt.out_key) is None and \
                FORMATS[pk.get("precision", L.PREC_FP32)].out_key in (None, fmt.out_key)
            cover.append((yt.ch_off, yt.ch_off + yt.C * yt.G))
        cover.sort()
        ok = ok and cover[0][0] == lo and cover[-1][1] == hi and all(cover[k][1] == cover[k + 1][0] for k in range(len(cover) - 1))
        if not ok:
            return False
        simg = kw["y"]                                   # the split image: compact, ld = xs.C * xs.G
        for t in writers:
            yt = self.ops[t][3]["y"]
            self._attach(t, fmt, T(simg.buf, yt.B, yt.H, yt.W, yt.C, yt.G, ld=simg.C * simg.G, ch_off=yt.ch_off - lo))
        return True

    def _fold_quant(self, i, kw, marks):
        """A quant whose input is the whole output of one MXFP8 conv, the tensor's only writer (VIDC_MXFP8_OUT: its epilogue writes the
        image).  Every other producer -- the max-pool, an upsample, Winograd outputs, the stem, a conv of another precision, several
        producers of one tensor, a channel slice -- is followed by the stand-alone quant launch."""
        fmt, xs = IMAGE_FORMATS["quant"], kw["x"]
        writers = [t for t in range(i) if xs.buf in self.ops[t][2]]
        if len(writers) != 1 or self.ops[writers[0]][0] != "conv":
            return False
        pk = self.ops[writers[0]][3]
        y = pk["y"]
        if FORMATS[pk["precision"]] is not fmt or pk.get(fmt.out_key) is not None or y.buf != xs.buf or \
                (y.ch_off, y.C, y.G, y.ld) != (xs.ch_off, xs.C, xs.G, xs.ld) or y.ch_off != 0 or y.ld != y.C * y.G:
            return False
        self._attach(writers[0], fmt, kw["y"])
        return True

    def _fold_cast(self, i, kw, marks):
        """A cast whose input is the whole output of one VIDC_PREC_BF16 conv, the last writer of the tensor before the cast and in the
        same segment (VIDC_BF16_OUT: its epilogue writes the image); not a Winograd GEMM.  Every other producer -- the max-pool, an
        upsample, the stem, a conv of another precision, producers of channel slices of a concat buffer -- is followed by the stand-alone
        cast launch."""
        fmt, xs = IMAGE_FORMATS["cast"], kw["x"]
        j = self._last_writer(i, xs.buf)
        if j is None or self.ops[j][0] != "conv":
            return False
        pk = self.ops[j][3]
        y = pk["y"]
        if FORMATS[pk["precision"]] is not fmt or pk.get(fmt.out_key) is not None or pk.get("wino") or y.buf != xs.buf or \
                (y.ch_off, y.C * y.G, y.ld) != (xs.ch_off, xs.C * xs.G, xs.ld) or y.ch_off != 0 or y.ld != y.C * y.G or \
                (y.B, y.H, y.W) != (xs.B, xs.H, xs.W) or self._cut_between(marks, j, i):
            return False
        self._attach(j, fmt, kw["y"])
        return True

    def _fuse_images(self):
        """An image op (split / quant / cast) is folded into the producer(s) of its input where the format's rule (_fold_<kind>) allows:
        their epilogues write the image.  A producer whose fp32 result nobody else reads then does not store it at all (VIDC_NO_F32_OUT,
        VIDC_UP_NO_F32_OUT, y = NULL; the output of a Bottleneck's last conv is the next block's residual and keeps its store)."""
        marks = {id(mk) for mk in self._cut_markers}
        n = len(self.ops)
        order = list(IMAGE_FORMATS)
        drop = {}                    # index of a folded image op -> the place of its format in the fold order
        for i, (kind, _r, _w, kw) in enumerate(self.ops):
            if kind in IMAGE_FORMATS and getattr(self, "_fold_" + kind)(i, kw, marks):
                drop[i] = order.index(kind)
        for j, (kind, _r, _w, kw) in enumerate(self.ops):
            place = next((k for k, fmt in enumerate(IMAGE_FORMATS.values()) if kw.get(fmt.out_key) is not None), None)
            if place is None or kw["y"].buf in self.pinned:
                continue
            # A later writer of the same buffer that accumulates into it needs the fp32 values too (reads cover that); a later plain
            # writer of ANOTHER slice of the buffer (stem groups) does not.  The formats fold one after the other -- all splits, then
            # all quants, then all casts -- so a folded image op of a LATER format still counts as a reader of this producer's result.
            yb = kw["y"].buf
            if not any(yb in self.ops[t][1] and drop.get(t, len(order)) > place for t in range(j + 1, n)):
                if kind in ("conv", "wino_out"):
                    kw["flags"] |= L.NO_F32_OUT
                elif kind == "upsample":
                    kw["flags"] |= L.UP_NO_F32_OUT
                else:
                    kw["no_f32"] = True
        self.n_fused_splits, self.n_fused_quants, self.n_fused_casts = (sum(1 for v in drop.values() if v == k) for k in range(len(order)))
        self.ops = [op for i, op in enumerate(self.ops) if i not in drop]

    def _fuse_warp_into_stem(self):
        """A stem conv whose input is the output of a forward warp that nothing else reads gathers its input through the warp itself
        (vidc_stem_conv3x3s2_warped: the tap sets of warp_fwd_kernel, bit for bit) and the warp launch + the warped image go away
        (VERDICT r4 item 9).  Not when the warped image has another reader (the use_mask branch, surface_normal.py:150-162) or is an output."""
        marks = {id(mk) for mk in self._cut_markers}
        drop = set()
        for i, (kind, reads, _w, kw) in enumerate(self.ops):
            if kind != "stem" or kw["x"].C != 3:
                continue
            xb = kw["x"].buf
            j = self._last_writer(i, xb)
            if j is None or self.ops[j][0] != "warp_fwd" or xb in self.pinned:
                continue
            if any(t != i and t not in drop and xb in self.ops[t][1] for t in range(len(self.ops))):
                continue
            if self._cut_between(marks, j, i):
                continue
            wkw = self.ops[j][3]
            kw["warp"] = {"x": wkw["x"], "p": wkw["p"], "intr": wkw["intr"], "ac": wkw["ac"]}
            self.ops[i] = (kind, [b for b in reads if b != xb] + [wkw["x"].buf, wkw["p"].buf], _w, kw)
            drop.add(j)
        self.ops = [op for t, op in enumerate(self.ops) if t not in drop]      # (the dropped warp ops are never cut markers, checked above)
        self.n_fused_warps = len(drop)

    def _conv_desc(self, kw, dry_run):
        """The vidc_conv_desc of a recorded conv (L.conv_desc / L.gemm_desc) with its tiling, and the op's display name."""
        x, y, keys, f = kw["x"], kw["y"], kw["keys"], kw["flags"]
        co, ci, kh, kwid, Ho, Wo = kw["geom"]
        prec, wm, wf, sig = kw["precision"], kw.get("wino", 0), kw.get("wino_fused", 0), kw["sig"]

        def addr(t):
            return self._addr(t) or None
        if wm:          # (m+2)^2 transform-domain GEMMs per group of the layer, identity epilogue shared by all of them
            wp = self.ws.packed_winograd(list(keys), wm, dry_run, prec)
            s1, b1 = self.ws.identity_affine(co, wp.device)
            s2 = b2 = None
            d = L.gemm_desc(x.W, ci, co, groups=len(keys) * (wm + 2) * (wm + 2), ldx=x.ld, ldy=y.ld, precision=prec, x=addr(x),
                            w=wp.data_ptr(), y=addr(y), scale1=s1.data_ptr(), shift1=b1.data_ptr())
        else:
            wp = self.ws.packed_winograd_fused(list(keys), dry_run) if wf else self.ws.packed(list(keys), dry_run, prec)
            s1, b1 = self.ws.affine(list(keys), list(kw["bn"]) if kw["bn"] is not None else None)
            s2, b2 = self.ws.affine([None] * len(keys), list(kw["bn2"])) if kw["bn2"] is not None else (None, None)
            r = kw["residual"]
            d = L.conv_desc(x.B, x.H, x.W, ci, co, kh, kwid, kw["stride"], kw["pad"], kw["dilation"], len(keys), Ho, Wo, x.ld, y.ld, prec,
                            x=addr(x), w=wp.data_ptr(), y=addr(y), scale1=s1.data_ptr(), shift1=b1.data_ptr(),
                            scale2=s2.data_ptr() if s2 is not None else None, shift2=b2.data_ptr() if b2 is not None else None,
                            relu1=f & L.RELU1, relu2=f & L.RELU2, residual=addr(r), ldr=r.ld if r is not None else None,
                            relu3=f & L.RELU3, accumulate=f & L.ACCUM, no_f32_out=f & L.NO_F32_OUT, wino_fused=bool(wf),
                            **{fmt.out_key: addr(kw.get(fmt.out_key)) for fmt in IMAGE_FORMATS.values()})
        self._keep += [t for t in (wp, s1, b1, s2, b2) if t is not None]
        if prec == L.PREC_MXFP8:        # no measured MXFP8 entries: the planner's tiling
            L.plan(d)
        elif prec == L.PREC_BF16:       # no measured bf16 entries either: the signature's measured tiling (the shape's best for the split-bf16
            ent = tuning_table().get(sig)                       # or fp32 kernel) where the bf16 kernel has that tile, else the planner's
            L.plan(d, (ent[0], ent[1]) if ent is not None and ent[0] in L.BF16_TILES else None)
        elif not wf:                    # the fused Winograd form has its own tile
            # the measured entry: [tile, splitk, precision] or [t, sk, prec, t32, sk32] with the best fp32 tiling as well; a 3-element entry
            # of the mixed mode sets the tiling of an fp32 conv of that signature too
            ent = tuning_table().get(sig)
            L.plan(d, None if ent is None else (ent[0], ent[1]) if len(ent) < 5 or prec == ent[2] else (ent[3], ent[4]))
        form = "@wino4f" if wf else ("@wino%d" % wm if wm else "")
        return d, "conv:%s%s:%s:sk%d:%s %s flags=0x%x" % (keys[0], form, L.TILE_NAMES[d.tile], d.splitk, FORMATS[prec].name, sig, d.flags)

    def _plan_buffers(self):
        n = len(self.buf_elems)
        multi_stream = any(kw["stream_id"] != 0 for _, _, _, kw in self.ops)
        storage = [None] * n
        if not self.reuse or multi_stream:
            for b in range(n):
                storage[b] = torch.zeros(max(self.buf_elems[b], 4), dtype=torch.float32, device=self.device)
            return storage
        last = [-1] * n
        first = [None] * n
        for i, (_, reads, writes, _) in enumerate(self.ops):
            for b in reads + writes:
                last[b] = i
                if first[b] is None:
                    first[b] = i
        free = []   # (elems, tensor)
        expire = {}
        for b in range(n):
            if b in self.pinned or first[b] is None:
                storage[b] = torch.zeros(max(self.buf_elems[b], 4), dtype=torch.float32, device=self.device)
            else:
                expire.setdefault(last[b], []).append(b)
        for i, (_, reads, writes, _) in enumerate(self.ops):
            for b in writes + reads:
                if storage[b] is None:
                    need = self.buf_elems[b]
                    best = None
                    for j, (el, _t) in enumerate(free):
                        if el >= need and (best is None or el < free[best][0]):
                            best = j
                    if best is not None:
                        storage[b] = free.pop(best)[1]
                    else:
                        storage[b] = torch.zeros(max(need, 4), dtype=torch.float32, device=self.device)
            for b in expire.get(i, []):
                free.append((storage[b].numel(), storage[b]))
        return storage

    # ---- lowering: _lower_<kind>(kw) returns the display name of the recorded op kw and the arguments of its entry point in the header's
    # declaration order, without the stream (L.pack_op puts them into slots) -- and the vidc_op_kind where it is not OP_KINDS[kind].
    # The lowerers of the ops that Program.variant_ops restricts take a window (g_lo, g_hi) of the groups of a grouped tensor: group g sits
    # at channel g * (channels per group) of every row, so a window moves the base addresses and shrinks the channel count.
    def _addr(self, t, extra=0):
        """Device address of the program tensor t (+ `extra` of its channels); 0 for no tensor."""
        return 0 if t is None else self.storage[t.buf].data_ptr() + t.esz * (t.ch_off + extra)

    def _lower(self, op, kind, kw, window=None):
        """Packs the recorded non-conv op kw into op.kind / op.u.g and returns its display name."""
        if kind in IMAGE_FORMATS:
            lowered = self._lower_image(kw, IMAGE_FORMATS[kind])
        else:
            lowered = getattr(self, "_lower_" + kind)(kw, *(() if window is None else (window,)))
        L.pack_op(op, lowered[2] if len(lowered) > 2 else OP_KINDS[kind], lowered[1])
        return lowered[0]

    def _lower_image(self, kw, fmt):
        """split / quant / cast: 64-bit row count, the channels of a row, the row stride of x, and the groups of a format that keeps them as planes."""
        x = kw["x"]
        rows, dims = x.B * x.H * x.W, ((x.C * x.G,) if fmt.folded else (x.C, x.G))
        return "%s:%s" % (fmt.kind, "x".join("%d" % v for v in (rows,) + dims)), (self._addr(x), self._addr(kw["y"]), rows, dims[0], x.ld) + dims[1:]

    def _lower_stem(self, kw):
        x, y, wf = kw["x"], kw["y"], kw.get("warp")
        w = self.ws.raw(kw["key"] + ".weight").contiguous()
        self._keep.append(w)
        out = (0 if kw.get("no_f32") else self._addr(y, kw["g"] * y.C), x.B, x.C, x.H, x.W, y.C, y.ld, int(kw["relu"]), self._addr(kw.get("split_out")), kw["g"] * y.C)
        if wf is None:
            return "stem:" + kw["key"], (self._addr(x), w.data_ptr()) + out
        # the input is gathered through the forward warp: the unwarped image and the parameter records in place of x; three channels, so no Cin
        return ("stem:" + kw["key"] + "+warp", (self._addr(wf["x"]), self._addr(wf["p"]), w.data_ptr(), out[0], out[1]) + out[3:] +
                (wf["intr"].cx, wf["intr"].cy, wf["ac"]), L.OP_STEM_WARPED)

    def _lower_maxpool(self, kw, window=None):
        x, y = kw["x"], kw["y"]
        g_lo, g_hi = window or (0, x.G)
        return "maxpool", (self._addr(x, g_lo * x.C), 0 if kw.get("no_f32") else self._addr(y, g_lo * x.C), x.B, x.H, x.W, x.C * (g_hi - g_lo), x.ld, y.ld,
                           self._addr(kw.get("split_out"), g_lo * x.C))

    def _lower_upsample(self, kw):
        x, y = kw["x"], kw["y"]
        return "upsample:%dx%dx%d->%dx%d" % (x.H, x.W, x.C * x.G, y.H, y.W), (
            self._addr(x), self._addr(y), x.B, x.H, x.W, (x.C if kw.get("sum_groups") else x.C * x.G), x.ld, y.H, y.W, y.ld, kw["flags"], self._addr(kw.get("split_out")))

    def _lower_head(self, kw):
        x, low, y = kw["x"], kw["low"], kw["y"]
        w = self.ws.raw(kw["key"] + ".weight").reshape(y.C, -1).contiguous()
        b = self.ws.raw(kw["key"] + ".bias").contiguous()
        self._keep += [w, b]
        return "head:" + kw["key"], (self._addr(x), w.data_ptr(), b.data_ptr(), self._addr(low), self._addr(y),
                                     x.B, x.H, x.W, x.C * x.G, x.ld, y.C, kw["pad"], y.H, y.W, int(kw["relu"]))

    def _lower_warp_params(self, kw):
        it = kw["intr"]
        return "warp_params", (self._addr(kw["g"]), self._addr(kw["a"]), self.B, it.fx, it.fy, it.cx, it.cy, self._addr(kw["kinv"]), it.W, it.H, self._addr(kw["p"]))

    def _lower_warp_fwd(self, kw):
        x, it = kw["x"], kw["intr"]
        return "warp_fwd", (self._addr(x), self._addr(kw["p"]), self._addr(kw["y"]), x.B, x.C, x.H, x.W, it.cx, it.cy, kw["ac"])

    def _lower_warp_inv(self, kw):
        x, it = kw["x"], kw["intr"]
        return "warp_inv_rot_norm", (self._addr(x), self._addr(kw["p"]), self._addr(kw["y"]), x.B, x.H, x.W, it.cx, it.cy, kw["ac"], kw["norm"])

    def _lower_avgpool(self, kw):
        x, y = kw["x"], kw["y"]
        return "avgpool", (self._addr(x), self._addr(y), x.B, x.H, x.W, x.C * x.G, x.ld) + tuple(kw["geom"]) + (y.ld,)

    def _lower_normalize(self, kw):
        x = kw["x"]
        return "normalize", (self._addr(x), self._addr(kw["y"]), x.B, x.C, x.H * x.W)

    def _lower_det_im2col(self, kw):
        return "det_im2col", (self._addr(kw["x"]), self._addr(kw["y"]), kw["x"].B) + tuple(kw["geom"]) + tuple(kw["mean"])

    def _lower_mask(self, kw):
        x, y, im = kw["x"], kw["y"], kw["image"]
        return "mask_scale", (self._addr(x), self._addr(im), self._addr(y), x.B, x.H, x.W, x.C * x.G, x.ld, y.ld, im.H, im.W)

    def _lower_wino_in(self, kw, window=None):
        x, v, cin, a2 = kw["x"], kw["v"], kw["cin"], (kw["m"] + 2) ** 2      # V rows: [group][position][cin] (row stride explicit)
        g_lo, C = (0, x.C * x.G) if window is None else (window[0], cin * (window[1] - window[0]))
        return "wino_in:F%d:%dx%dx%d" % (kw["m"], x.H, x.W, x.C * x.G), (
            self._addr(x, g_lo * cin), self._addr(v, g_lo * a2 * cin), x.B, x.H, x.W, C, x.ld, cin, kw["m"], kw["split"], v.ld)

    def _lower_wino_out(self, kw, window=None):
        mm, y, keys, co, a2 = kw["mm"], kw["y"], kw["keys"], kw["cout"], (kw["m"] + 2) ** 2
        s1, b1 = self.ws.affine(list(keys), list(kw["bn"]) if kw["bn"] is not None else None)
        s2, b2 = self.ws.affine([None] * len(keys), list(kw["bn2"])) if kw["bn2"] is not None else (None, None)
        if window is None:
            self._keep += [t for t in (s1, b1, s2, b2) if t is not None]
        g_lo, C = (0, y.C * y.G) if window is None else (window[0], co * (window[1] - window[0]))
        # M rows: [group][position][cout]; y, its split image and the scale / shift arrays: group g at element g * cout
        return "wino_out:F%d:%dx%dx%d" % (kw["m"], y.H, y.W, y.C * y.G), (
            self._addr(mm, g_lo * a2 * co), 0 if kw["flags"] & L.NO_F32_OUT else self._addr(y, g_lo * co), self._addr(kw.get("split_out"), g_lo * co)) + tuple(
            0 if t is None else t.data_ptr() + 4 * g_lo * co for t in (s1, b1, s2, b2)) + (y.B, y.H, y.W, C, co, y.ld, kw["m"], kw["flags"], mm.ld)

    def _lower_nearest2x(self, kw):
        x, y = kw["x"], kw["y"]
        return "nearest2x", (self._addr(x), self._addr(y), x.B, x.H, x.W, x.C * x.G, x.ld, y.ld)

    def _lower_copy(self, kw):
        src, dst = kw["src"], kw["dst"]
        return "copy", (self._addr(src), self._addr(dst), min(self.buf_elems[src.buf], self.buf_elems[dst.buf]) * 4)

    def finalize(self, dry_run=False):
        """Plans buffers and builds the C op array.  dry_run=True stops before any HIP call (host-logic tests on CPU)."""
        lib = L.lib()
        # Opt-in (VIDC_FUSE_WARP=1): bit-identical, one launch and 2 x 3HW x 4 bytes less per frame, no measurable gain (< 0.2 % of the tick).  (The wrong
        # frames round 5 saw with it were an execution defect of a packed-fp32 instruction beside bf16 MFMAs, not this kernel's loads: DESIGN 4.5.)
        if os.environ.get("VIDC_FUSE_WARP", "0") == "1":
            self._fuse_warp_into_stem()
        if os.environ.get("VIDC_FUSE_SPLIT", "1") == "1":
            self._fuse_images()
        self.cuts = [next(i for i, op in enumerate(self.ops) if op is mk) + 1 for mk in self._cut_markers]
        assert len(self.cuts) < L.MAX_SEGMENTS and self.cuts == sorted(set(self.cuts))
        self.storage = self._plan_buffers()
        self.bytes_allocated = sum({t.data_ptr(): t.numel() * 4 for t in self.storage if t is not None}.values())
        ops = (L.Op * len(self.ops))()
        ws_need = {}
        ws_ops = []              # the convs that need a split-K workspace
        self.op_names = []
        for op, (kind, _r, _w, kw) in zip(ops, self.ops):
            if kind not in OP_KINDS:
                raise ValueError(kind)
            op.stream_id, op.wait_mask = kw["stream_id"], kw["wait_mask"]
            if kind == "conv":
                op.kind = L.OP_CONV
                op.u.conv, name = self._conv_desc(kw, dry_run)
                need = lib.vidc_conv2d_workspace_bytes(C.byref(op.u.conv))
                if need:
                    ws_need[op.stream_id] = max(ws_need.get(op.stream_id, 0), need)
                    ws_ops.append(op)
            else:
                name = self._lower(op, kind, kw)
            self.op_names.append(name)
        # split-K workspaces (one per stream id so concurrent convs never share partials); zeroed once: their heads hold the
        # per-tile ticket counters of the fused split-K reduction, which every launch leaves at zero (include/vidc.h)
        self.workspaces = {sid: torch.zeros(nb // 4 + 4, dtype=torch.float32, device=self.device) for sid, nb in ws_need.items()}
        for op in ws_ops:
            op.u.conv.workspace = self.workspaces[op.stream_id].data_ptr()
        self.c_ops = ops
        self.captured = False
        if dry_run:
            return self
        h = C.c_void_p()
        L.check(lib.vidc_program_create(ops, len(ops), C.byref(h)), "program_create")
        self.handle = h
        self.captured = False
        # The pack / fold kernels above ran on the stream that was current while this program was built, and their results are
        # cached in the WeightStore: a program built later for another slot launches on ANOTHER stream and must not race them.
        # One host wait here (not on the hot path) orders every later consumer after the packing.
        torch.cuda.current_stream(self.device).synchronize()
        return self

    # ---- execution ----------------------------------------------------------------------------------------
    def tensor(self, t):
        """torch view of a program tensor (NCHW tensors come back shaped (B,C,H,W))."""
        s = self.storage[t.buf]
        if t.nchw:
            return s[: t.B * t.C * t.H * t.W].view(t.B, t.C, t.H, t.W)
        return s[: t.B * t.H * t.W * t.ld].view(t.B, t.H, t.W, t.ld)[..., t.ch_off: t.ch_off + t.C * t.G]

    def run(self, stream=None):
        L.check(L.lib().vidc_program_run(self.handle, stream if stream is not None else L.current_stream()), "program_run")

    def capture(self, stream=None):
        L.check(L.lib().vidc_program_capture(self.handle, stream if stream is not None else L.current_stream()), "program_capture")
        self.captured = True

    def segments(self):
        """[(begin, end)] op ranges separated by cut()."""
        edges = [0] + list(self.cuts) + [len(self.ops)]
        return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]

    def run_segment(self, k, stream=None):
        b, e = self.segments()[k]
        L.check(L.lib().vidc_program_run_range(self.handle, stream if stream is not None else L.current_stream(), b, e), "program_run_range")

    def capture_segments(self, stream=None):
        st = stream if stream is not None else L.current_stream()
        for k, (b, e) in enumerate(self.segments()):
            L.check(L.lib().vidc_program_capture_range(self.handle, st, b, e, k), "program_capture_range")
        self.captured = True

    def launch_segment(self, k, stream=None):
        L.check(L.lib().vidc_program_launch_segment(self.handle, stream if stream is not None else L.current_stream(), k), "program_launch_segment")

    def launch(self, stream=None):
        L.check(L.lib().vidc_program_launch(self.handle, stream if stream is not None else L.current_stream()), "program_launch")

    # ---- group-restricted variants of a segment ---------------------------------------------------------------------------
    def group_variant(self, name, segment, g_lo, g_hi, groups, keep_ungrouped):
        """A second native program over the SAME buffers, packed weights and tile choices: the ops of `segment` with every
        `groups`-group launch (fused convs, the max-pool over the grouped stem output, the per-group stem kernels) restricted to groups
        [g_lo, g_hi), and the segment's other ops kept or dropped.  pipeline.build_frame_program's tick runs the surface-normal pyramid
        (group 0) and the three depth-completion pyramids (groups 1..3) as 4-group launches; the first tick of a frame stream has no
        previous frame to complete and the drain tick no new one to start, so they run the variants (0, 1, keep) / (1, 4, drop) and the
        chip does the work of exactly n frames for n frames.  Per output element nothing changes: a group only selects base pointers
        (csrc/conv_mfma.hip: `a.x + g * a.x_gs` ...), while tile, split-K partition and K order -- which fix the fp32 summation order --
        are copied from the grouped launch.  So a frame's result is bit-identical whichever variant computed its pyramids
        (tests/test_hip_parity.py::test_run_interleaved_lanes_are_bit_identical)."""
        assert self.handle is not None
        ops, picked = self.variant_ops(segment, g_lo, g_hi, groups, keep_ungrouped)
        h = C.c_void_p()
        L.check(L.lib().vidc_program_create(ops, len(ops), C.byref(h)), "program_create (variant)")
        self._variants = getattr(self, "_variants", {})
        self._variants[name] = {"handle": h, "ops": ops, "captured": False, "indices": picked}
        return self._variants[name]

    def variant_ops(self, segment, g_lo, g_hi, groups, keep_ungrouped):
        """(the op array of group_variant's program, the indices of the ops of this program it was made from): needs a finalized program,
        dry-run included."""
        assert 0 <= g_lo < g_hi <= groups
        b, e = self.segments()[segment]
        picked = []

        def grouped(kind, kw):
            return (kind in ("conv", "wino_out") and len(kw["keys"]) == groups) or (kind in ("maxpool", "wino_in") and kw["x"].G == groups)
        for i in range(b, e):
            kind, _r, _w, kw = self.ops[i]
            if kind == "stem":
                if g_lo <= kw["g"] < g_hi:
                    picked.append(i)
                continue
            # (a split launch of its own -- VIDC_FUSE_SPLIT=0 -- over a grouped tensor has no row stride for its image: it runs whole in every variant)
            if grouped(kind, kw) or keep_ungrouped or (kind in IMAGE_FORMATS and kw["x"].G == groups):
                picked.append(i)
        ops = (L.Op * len(picked))()
        for j, i in enumerate(picked):
            C.memmove(C.byref(ops[j]), C.byref(self.c_ops[i]), C.sizeof(L.Op))
            kind, _r, _w, kw = self.ops[i]
            if not grouped(kind, kw):
                continue
            if kind == "conv":
                d = ops[j].u.conv
                a2 = (kw["wino"] + 2) ** 2 if kw.get("wino") else 1        # Winograd GEMMs: (m+2)^2 launch groups per group of the layer
                strides = [("x", d.x_gs, 4), ("w", d.w_gs, 4), ("y", d.y_gs, 4), ("scale1", d.p_gs, 4), ("shift1", d.p_gs, 4), ("scale2", d.p_gs, 4),
                           ("shift2", d.p_gs, 4), ("residual", d.r_gs, 4)]                           # these operands are 4 bytes per element
                strides += [("y_split", fmt.out_gs(d), fmt.out_esz) for fmt in IMAGE_FORMATS.values() if d.flags & fmt.out_flag]
                for field, gs, esz in strides:
                    v = getattr(d, field)
                    if v:
                        setattr(d, field, v + esz * g_lo * gs * a2)
                d.groups = (g_hi - g_lo) * a2
            else:                # max-pool, wino_in, wino_out: lowered again with the window (stream id and wait mask are the copied ones)
                self._lower(ops[j], kind, kw, (g_lo, g_hi))
        return ops, picked

    def has_variant(self, name):
        return name in getattr(self, "_variants", {})

    def run_variant(self, name, stream=None):
        L.check(L.lib().vidc_program_run(self._variants[name]["handle"], stream if stream is not None else L.current_stream()), "variant_run")

    def capture_variant(self, name, stream=None):
        v = self._variants[name]
        L.check(L.lib().vidc_program_capture(v["handle"], stream if stream is not None else L.current_stream()), "variant_capture")
        v["captured"] = True

    def launch_variant(self, name, stream=None):
        v = self._variants[name]
        st = stream if stream is not None else L.current_stream()
        if v["captured"]:
            L.check(L.lib().vidc_program_launch(v["handle"], st), "variant_launch")
        else:
            L.check(L.lib().vidc_program_run(v["handle"], st), "variant_run")

    def time(self, iters=20, use_graph=False, per_op=False, stream=None):
        ms = (C.c_float * 1)()
        per = (C.c_float * len(self.ops))() if per_op else None
        L.check(L.lib().vidc_program_time(self.handle, stream if stream is not None else L.current_stream(), iters,
                                          int(use_graph), ms, per), "program_time")
        return (ms[0], list(per)) if per_op else ms[0]

    def __del__(self):
        try:
            if self.handle is not None:
                L.lib().vidc_program_destroy(self.handle)
            for v in getattr(self, "_variants", {}).values():
                L.lib().vidc_program_destroy(v["handle"])
        except Exception:
            pass
