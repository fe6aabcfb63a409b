"""Every non-conv op kind of a Program, run as a one-op program packed by _lib.pack_op, against the same entry point called directly
through ctypes with the same arguments: the same kernel on the same inputs, so every output buffer -- guard region included -- must hold
the same BYTES.  Any difference is a packing error (csrc/program.hip's slot walk, or pack_op's), so there is no tolerance.

Shapes are the smallest that tell slots apart: B = 2, all extents of a case pairwise different (a swapped pair changes the result or is
refused), ld > C wherever the entry takes a row stride.  Where a header rule forbids the obvious shape the case says so.  Outputs are
pre-filled with NaN bytes; an output that the kernel accumulates into starts from the same data in both runs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                       # untouchable floats behind every output
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX, FY, CX, CY = 7.25, 6.5, 3.75, 2.875       # pinhole intrinsics of a 6 x 8 image, pairwise different


def _L():
    from vi_depth_completion_amd import _lib as L
    return L


class _Case:
    """The buffers of one case: inputs made once (by name) and shared by the two runs, outputs fresh per run."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.inputs = {}
        self.outs = None

    def inp(self, name, *shape, data=None):
        if name not in self.inputs:
            t = torch.randn(*shape, generator=self.gen) if data is None else torch.as_tensor(data, dtype=torch.float32)
            self.inputs[name] = t.contiguous().to(DEV)
        return self.inputs[name]

    def out(self, n, init=None):
        """n floats of NaN (+ GUARD); `init`: what the first n hold instead (an output that is accumulated into)."""
        t = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        if init is not None:
            t[:n] = init.reshape(-1)
        self.outs.append(t)
        return t


def _params(c, H, W, fx, fy, cx, cy):
    """Warp parameter records of a near-upright and a strongly tilted gravity (tests/golden/warp_cases.npz), made once per case by the entry itself."""
    if "params" not in c.inputs:
        L = _L()
        cases = np.load(os.path.join(GOLDEN, "warp_cases.npz"))
        g, a = c.inp("gravity", data=cases["gravity"][[2, 9]]), c.inp("aligned", data=cases["aligned"][[2, 9]])
        kinv = c.inp("kinv", data=np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])).astype(np.float32).reshape(-1))
        p = torch.zeros(2 * L.WARP_PARAMS, dtype=torch.float32, device=DEV)
        L.check(L.lib().vidc_warp2dof_params(L.ptr(g), L.ptr(a), 2, fx, fy, cx, cy, L.ptr(kinv), W, H, L.ptr(p), L.current_stream()), "warp params")
        c.inputs["params"] = p
    return c.inputs["params"]


# ---- one function per case: (op kind, the entry's arguments in declaration order without the stream; tensors stand for their addresses) ----
def _stem(c, warped=False, align_corners=0):
    B, Cin, H, W, Cout, ldy, ch0 = 2, 3, 4, 6, 32, 64, 32                      # -> Ho x Wo = 2 x 3; the slice [32, 64) of a 64-channel tensor
    L = _L()
    x, w = c.inp("x", B, Cin, H, W), c.inp("w", Cout, Cin, 3, 3)
    rows = B * 2 * 3
    y, image = c.out(rows * ldy), c.out(rows * ldy)                             # the split image of the whole tensor: 128 bytes per 32 channels
    tail = (y.data_ptr() + 4 * ch0, B) + ((H, W) if warped else (Cin, H, W)) + (Cout, ldy, 1, image, ch0)
    if not warped:
        return L.OP_STEM, (x, w) + tail
    sx, sy = W / 8.0, H / 6.0
    intr = (FX * sx, FY * sy, CX * sx, CY * sy)
    return L.OP_STEM_WARPED, (x, _params(c, H, W, *intr), w) + tail + (intr[2], intr[3], align_corners)


def _maxpool(c, split):
    B, H, W, Cn, ldx, ldy = 2, 5, 7, 32, 64, 96                                 # -> 3 x 4
    x = c.inp("x", B, H, W, ldx)
    return _L().OP_MAXPOOL, (x, c.out(B * 3 * 4 * ldy), B, H, W, Cn, ldx, ldy, c.out(B * 3 * 4 * ldy) if split else None)


def _upsample(c):
    B, h, w, Cn, ldx, H, W, ldy = 2, 3, 5, 32, 64, 7, 9, 96
    L = _L()
    x, base = c.inp("x", B, h, w, ldx), c.inp("base", B * H * W * ldy)           # ACCUM adds onto what y holds
    return L.OP_UPSAMPLE, (x, c.out(B * H * W * ldy, init=base), B, h, w, Cn, ldx, H, W, ldy, L.UP_RELU | L.UP_ACCUM, None)


def _head(c):
    B, h, w, Cin, ldx, Cout, pad, H, W = 2, 3, 4, 64, 96, 1, 1, 7, 9
    x, wt, bias = c.inp("x", B, h, w, ldx), c.inp("w", Cout, Cin), c.inp("bias", Cout)
    return _L().OP_HEAD, (x, wt, bias, c.out(B * Cout * (h + 2 * pad) * (w + 2 * pad)), c.out(B * Cout * H * W), B, h, w, Cin, ldx, Cout, pad, H, W, 1)


def _warp_params(c):
    cases = np.load(os.path.join(GOLDEN, "warp_cases.npz"))
    g, a = c.inp("gravity", data=cases["gravity"][[2, 9]]), c.inp("aligned", data=cases["aligned"][[2, 9]])
    kinv = c.inp("kinv", data=np.linalg.inv(np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])).astype(np.float32).reshape(-1))
    return _L().OP_WARP_PARAMS, (g, a, 2, FX, FY, CX, CY, kinv, 8, 6, c.out(2 * _L().WARP_PARAMS))


def _warp_fwd(c):
    B, Cn, H, W = 2, 3, 6, 8
    return _L().OP_WARP_FWD, (c.inp("x", B, Cn, H, W), _params(c, H, W, FX, FY, CX, CY), c.out(B * Cn * H * W), B, Cn, H, W, CX, CY, 0)


def _warp_inv(c):
    B, H, W = 2, 6, 8
    return _L().OP_WARP_INV, (c.inp("x", B, 3, H, W), _params(c, H, W, FX, FY, CX, CY), c.out(B * 3 * H * W), B, H, W, CX, CY, 0, 1)


def _image(c, kind):
    """split / cast: rows 35, C 32 / 64, ldx = C + 32.  quant: C 128 in 2 groups; the header wants ldx >= groups * C, so ldx = 2 * 128 + 32
    in place of C + 32.  Image sizes: 4 bytes per channel (split), 2 (cast), 33 bytes per 32 channels (quant)."""
    L = _L()
    rows = 35
    if kind == "split":
        return L.OP_SPLIT, (c.inp("x", rows, 64), c.out(rows * 32), rows, 32, 64)
    if kind == "cast":
        return L.OP_CAST, (c.inp("x", rows, 96), c.out(rows * 64 // 2), rows, 64, 96)
    return L.OP_QUANT, (c.inp("x", rows, 288), c.out(-(-2 * rows * 128 * 33 // 128)), rows, 128, 288, 2)


def _avgpool(c):
    B, H, W, Cn, ldx, ldy = 2, 5, 7, 32, 64, 96                                 # kernel (2, 3), stride (1, 2), padding (0, 1) -> 4 x 4
    return _L().OP_AVGPOOL, (c.inp("x", B, H, W, ldx), c.out(B * 4 * 4 * ldy), B, H, W, Cn, ldx, 2, 3, 1, 2, 0, 1, ldy)


def _normalize(c):
    return _L().OP_NORMALIZE, (c.inp("x", 2, 3, 35), c.out(2 * 3 * 35), 2, 3, 35)


def _det_im2col(c):
    """The 5 x 7 image of tests/test_detector_kernels.py, padded to 6 x 8 (any even Hp >= H, Wp >= W is allowed; the detector's own padding
    to 32 x 32 would not tell Hp from Wp): cols [2][3][4][160]."""
    img = c.inp("x", data=torch.rand(2, 3, 5, 7, generator=c.gen))
    return _L().OP_DET_IM2COL, (img, c.out(2 * 3 * 4 * 160), 2, 5, 7, 6, 8, 102.9801, 115.9465, 122.7717)


def _nearest2x(c):
    B, h, w, Cn, ldx, ldy = 2, 5, 7, 4, 8, 12                                   # the smallest strided case of tests/test_detector_kernels.py
    return _L().OP_NEAREST2X, (c.inp("x", B, h, w, ldx), c.out(B * 2 * h * 2 * w * ldy), B, h, w, Cn, ldx, ldy)


def _mask(c):
    B, h, w, Cn, ldx, ldy, H, W = 2, 3, 5, 32, 64, 96, 6, 8                      # (tests/test_detector_kernels.py has no case of this entry)
    img = c.inp("image", data=torch.rand(B, 3, H, W, generator=c.gen) * (torch.rand(B, 1, H, W, generator=c.gen) > 0.4))      # empty where the mask is 0
    return _L().OP_MASK, (c.inp("x", B, h, w, ldx), img, c.out(B * h * w * ldy), B, h, w, Cn, ldx, ldy, H, W)


def _wino_in(c):
    B, H, W, Cin, G, ldx, m = 2, 5, 7, 32, 2, 96, 4                              # 2 x 2 tiles per image; V rows of 36 * 64 values, stride 64 more
    ldv = 36 * G * Cin + 64
    return _L().OP_WINO_IN, (c.inp("x", B, H, W, ldx), c.out(B * 2 * 2 * ldv), B, H, W, G * Cin, ldx, Cin, m, 0, ldv)


def _wino_out(c):
    B, Ho, Wo, Cout, G, ldy, m = 2, 5, 7, 32, 2, 96, 4
    L = _L()
    ldm = 36 * G * Cout + 32
    mm = c.inp("mm", B * 2 * 2, ldm)
    affine = [c.inp(k, G * Cout) for k in ("scale1", "shift1", "scale2", "shift2")]
    return L.OP_WINO_OUT, (mm, c.out(B * Ho * Wo * ldy), None, *affine, B, Ho, Wo, G * Cout, Cout, ldy, m, L.RELU1 | L.AFFINE2 | L.RELU2, ldm)


def _copy(c):
    return _L().OP_COPY, (c.inp("src", 1024), c.out(1024 - GUARD), 1000)       # 1000 bytes between two 4096-byte buffers


CASES = {
    "stem": _stem, "stem_warped": lambda c: _stem(c, True, 0), "stem_warped_align_corners": lambda c: _stem(c, True, 1),
    "maxpool": lambda c: _maxpool(c, False), "maxpool_split": lambda c: _maxpool(c, True), "upsample": _upsample, "head": _head,
    "warp_params": _warp_params, "warp_fwd": _warp_fwd, "warp_inv": _warp_inv,
    "split": lambda c: _image(c, "split"), "cast": lambda c: _image(c, "cast"), "quant": lambda c: _image(c, "quant"),
    "avgpool": _avgpool, "normalize": _normalize, "det_im2col": _det_im2col, "nearest2x": _nearest2x, "mask": _mask,
    "wino_in": _wino_in, "wino_out": _wino_out, "copy": _copy,
}


class _NoDevice(_Case):
    """Case buffers without a device: for reading a case's op kind and argument count."""

    def __init__(self):
        super().__init__(0)
        self.inputs["params"] = torch.zeros(1)

    def inp(self, name, *shape, data=None):
        return self.inputs.setdefault(name, torch.zeros(1))

    def out(self, n, init=None):
        return torch.zeros(1)


def test_the_cases_cover_every_generic_kind():
    """(No GPU.)  Every op kind but the conv has a case, and a case passes as many arguments as its entry's ctypes signature without the stream."""
    L = _L()
    cases = [CASES[name](_NoDevice()) for name in CASES]
    assert {kind for kind, _args in cases} == set(range(2, 22)) - {15}
    entry = {L.OP_STEM: "vidc_stem_conv3x3s2", L.OP_STEM_WARPED: "vidc_stem_conv3x3s2_warped", L.OP_MAXPOOL: "vidc_maxpool3x3s2",
             L.OP_UPSAMPLE: "vidc_upsample_bilinear_ac", L.OP_HEAD: "vidc_head_conv1x1_upsample", L.OP_WINO_OUT: "vidc_winograd_output_transform"}
    for kind, args in cases:
        if kind in entry:
            assert len(args) == len(L.SIGNATURES[entry[kind]][1]) - 1, kind


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_op_equals_the_direct_call(name):
    L = _L()
    lib, st = L.lib(), L.current_stream()
    c = _Case(sum(map(ord, name)))
    runs = []
    for _ in range(2):
        c.outs = []
        kind, args = CASES[name](c)
        runs.append((tuple(L.ptr(a) if isinstance(a, torch.Tensor) else a for a in args), c.outs))
    (packed_args, packed_outs), (direct_args, direct_outs) = runs
    # the program: one op, packed from the argument tuple by the class string the library reports
    ops = (L.Op * 1)()
    L.pack_op(ops[0], kind, packed_args)
    h = C.c_void_p()
    L.check(lib.vidc_program_create(ops, 1, C.byref(h)), "program_create")
    try:
        L.check(lib.vidc_program_run(h, st), "program_run")
    finally:
        torch.cuda.synchronize()
        lib.vidc_program_destroy(h)
    # the same entry, called directly
    e = L.OpEntry()
    L.check(lib.vidc_op_info(kind, C.byref(e)), "op_info")
    if kind == L.OP_COPY:      # (the program's own copy function is not exported)
        src, dst, nbytes = c.inputs["src"], direct_outs[0], direct_args[2]
        dst.view(torch.uint8)[:nbytes] = src.view(torch.uint8)[:nbytes]
    else:
        L.check(getattr(lib, e.name)(*direct_args, st), e.name)
    torch.cuda.synchronize()
    assert len(packed_outs) == len(direct_outs) >= 1
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    for a, b in zip(packed_outs, direct_outs):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert (b.view(torch.int32)[:-GUARD] != nan_bits).any(), "the direct call wrote nothing"
        assert (b.view(torch.int32)[-GUARD:] == nan_bits).all(), "the guard region was written"
