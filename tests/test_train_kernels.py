"""The row kernels of the training step (csrc/train.hip), one by one, at the smallest shapes that reach each of their branches.

The trainers reach the train-mode BatchNorm, its backward, their per-channel reductions and the elementwise / layout helpers only through
composites on tidy shapes, compared at 2e-4 .. 1e-2 of a tensor's scale.  Here every kernel is called through the C ABI on shapes
(M rows, C channels, row stride ld) chosen for the branches: more than 32 reduction chunks, a chunk count that is no multiple of 32,
C % 64 != 0, M % 64 != 0 and M % 16 != 0, ld > C with a different stride per tensor, the Mp zero padding of the transposed bf16 copy,
dx == NULL, and the 8-wide body against the scalar tail of the gradient casts.

References are float64 and read only the fp32 inputs of the kernel under test.  Bounds are elementwise forward-error bounds built from the
reference's own float64 magnitudes (u = 2^-24, the unit roundoff of fp32), never from the kernel's output or a fraction of a tensor's
maximum, so a constant channel (y - beta and dx are pure cancellation) and a channel whose ReLU gates are all closed are held to the same
bounds as every other.  A CPU test checks the references themselves against torch.autograd in float64.

Counted roundings behind each factor (reading the kernels; measured ratios: profiles/EXPERIMENTS.md):
  y          8u (|x a| + |mu a| + |beta| + |res|)        a = fl(rstd * gamma): 2u; fl(mean * a): 4u of |mu a|; two sums, one per term
  save_mean  2u |mu|, save_rstd 2u rstd                  fp64 moments, one rounding each
  running    2u (|old| + |momentum * new|)               fp64, one rounding
  dx         8u |gamma rstd| (|g'| + |S g'| / M + 2 |xh| |S g' xh| / M)  +  2u |gamma rstd| |xh| S |g' xh| / M
  dgamma     4u S |g' xh|                                xh is an fp32 value (2u), the sum fp64, one rounding
  dbeta, column sums   2u S |.|                          fp64 sum, one rounding

The second term of dx is the one rounding the first derivation miscounted.  chan_partial_kernel forms xh = fl(fl(x - mean) * rstd) in fp32
before it adds g' * xh up in fp64, so the sum S g' xh carries an error of up to 2u S |g' xh| -- exactly what the dgamma bound budgets --
and dx inherits it times |gamma rstd| |xh| / M.  The first derivation charged that error to |S g' xh|, which is arbitrarily smaller than
S |g' xh| where the sum cancels (a channel whose dgamma happens to be near 0), so no integer factor on that term is a bound; the term
added here is the counted one (the two roundings of xh), built like all others from the reference's magnitudes.  Measured on MI355X over
the shapes below: largest error / bound 2.14 without the term (shape (257, 132, 160); 1.29 at (63, 68, 72): a row with a closed gate and
|xh| = 3.0 in a channel with |S g' xh| = 0.004 S |g' xh|), 0.44 with it.  Every other bound held as first derived (largest ratio 0.49).
"""
import hashlib
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))            # the kernels take eps and momentum as fp32: the references read those values
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))
SENTINEL = -7777.0                                              # what the ld - C gap of every output row holds before a call
F64 = torch.float64

# (M, C, ld) and the number of reduction chunks chan_partial_kernel makes of it
SHAPES = [
    (2, 4, 8),            # smallest legal shape
    (17, 8, 12),          # one row past the 16 row-lanes of a reduction block, M < 64
    (63, 68, 72),         # a second channel block of 4 channels, M < 64
    (65, 64, 64),         # one row into the second pixel block
    (257, 132, 160),      # three channel blocks, the last one partial
    (2000, 4, 4),         # 63 chunks of 32 rows: two rounds of 32, the second clamped; fold offered (32 pixel blocks * 63 <= 4096)
    (2000, 68, 100),      # two channel blocks; 63 chunks as well (rows_for counts both channel blocks: 4000 / 512 -> 32 rows)
    (1000, 68, 100),      # 32 chunks exactly: one unclamped round, the last chunk 8 rows; fold offered
    (20000, 8, 8),        # 417 chunks of 48 rows: 14 rounds in chan_final_kernel; fold NOT offered (313 * 417 > 4096)
]
CHUNKS = {(2000, 4, 4): 63, (2000, 68, 100): 63, (1000, 68, 100): 32, (20000, 8, 8): 417}
_IDS = ["%dx%d_ld%d" % s for s in SHAPES]


# ---- Python restatement of rows_for / chunks_for / fold_bn (csrc/train.hip) ------------------------------------------------------------
def _rows_for(M, C):
    r = (M * ((C + 63) // 64) + 511) // 512
    r = (r + 15) // 16 * 16
    return min(max(r, 32), 256)


def _chunks_for(M, C):
    r = _rows_for(M, C)
    return (M + r - 1) // r


def _fold_offered(M, C):
    return M < 2 ** 31 and ((M + 63) // 64) * _chunks_for(M, C) <= 4096


def _lib_chunks(lib, M, C):
    """The chunk count behind vidc_train_scratch_bytes = (chunks * 2C + 2C) doubles + 256."""
    doubles, rem = divmod(lib.vidc_train_scratch_bytes(M, C) - 256, 8)
    n, rem2 = divmod(doubles - 2 * C, 2 * C)
    assert rem == 0 and rem2 == 0
    return n


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def ref_bn_forward(x, gamma, beta, eps, momentum, relu, res=None, running_mean=None, running_var=None):
    """nn.BatchNorm2d in train() over the rows of x [M][C] (+ residual, + ReLU).  Returns the values and, per quantity, the magnitude
    `*_mag` its bound multiplies (the sum of the absolute values of the terms that are rounded)."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    M = x.shape[0]
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    alpha = rstd * gamma
    y = x * alpha + (beta - mu * alpha)
    y_mag = (x * alpha).abs() + (mu * alpha).abs() + beta.abs()
    if res is not None:
        y = y + res.to(F64)
        y_mag = y_mag + res.to(F64).abs()
    if relu:
        y = y.clamp_min(0.0)
    out = dict(mu=mu, var=var, rstd=rstd, y=y, y_mag=y_mag, mu_mag=mu.abs(), rstd_mag=rstd)
    if running_mean is not None:
        unbiased = var * M / (M - 1) if M > 1 else var           # (M == 1: the kernel's documented choice, torch refuses the call)
        rm, rv = running_mean.to(F64), running_var.to(F64)
        out.update(rm=(1.0 - momentum) * rm + momentum * mu, rv=(1.0 - momentum) * rv + momentum * unbiased,
                   rm_mag=rm.abs() + (momentum * mu).abs(), rv_mag=rv.abs() + (momentum * unbiased).abs())
    return out


def ref_bn_backward(dy, x, y_relu, gamma, save_mean, save_rstd):
    """From the GIVEN mean and invstd (inputs of the backward): g' = dy * (y_relu > 0), xh = (x - mean) * rstd, dbeta = S g',
    dgamma = S g' xh, dx = gamma rstd (g' - dbeta / M - xh dgamma / M)."""
    dy, x, gamma, mean, rstd = dy.to(F64), x.to(F64), gamma.to(F64), save_mean.to(F64), save_rstd.to(F64)
    M = x.shape[0]
    g = dy if y_relu is None else dy * (y_relu > 0).to(F64)
    xh = (x - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    dx = gamma * rstd * (g - dbeta / M - xh * dgamma / M)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta,
                dx_mag=(gamma * rstd).abs() * (g.abs() + dbeta.abs() / M + 2.0 * xh.abs() * dgamma.abs() / M),
                dx_sum_mag=(gamma * rstd).abs() * xh.abs() * (g * xh).abs().sum(0) / M,      # (see the module docstring: the rounding inside S g' xh)
                dgamma_mag=(g * xh).abs().sum(0), dbeta_mag=g.abs().sum(0))


def ref_colsum(a):
    a = a.to(F64)
    return a.sum(0), a.abs().sum(0)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
class _Data:
    """Seeded normal data per channel; with C >= 8 three special channels: `offset` (mean 100, sigma 0.1), `const` (3.25 in every row, in
    the last -- partial -- channel block) and `neg` (all negative; its ReLU gates are all closed in the backward's y_relu)."""

    def __init__(self, M, C):
        g = torch.Generator().manual_seed(1000 * M + C)
        self.M, self.C = M, C
        x = torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + torch.randn(C, generator=g)
        self.offset = self.const = self.neg = None
        if C >= 8:
            self.offset, self.const, self.neg = 1, C - 1, C - 3
            x[:, self.offset] = 100.0 + 0.1 * torch.randn(M, generator=g)
            x[:, self.const] = 3.25
            x[:, self.neg] = -(torch.randn(M, generator=g).abs() + 0.5)
        self.x = x
        self.dy = torch.randn(M, C, generator=g)
        self.res = torch.randn(M, C, generator=g)
        self.gamma = torch.rand(C, generator=g) + 0.5
        self.beta = torch.randn(C, generator=g) * 0.2
        self.rm = torch.randn(C, generator=g) * 0.5
        self.rv = torch.rand(C, generator=g) + 0.5


_DATA = {}


def _data(M, C):
    if (M, C) not in _DATA:
        _DATA[(M, C)] = _Data(M, C)
    return _DATA[(M, C)]


def _strides(C, ld):
    """Four row strides for the tensors of one call: all dense where the table says ld == C, else four different ones from ld on."""
    return (C,) * 4 if ld == C else (ld, ld + 4, ld + 8, ld + 12)


def _rows(t, ld, fill=float("nan")):
    """t [M][C] as device rows of stride ld; the gap holds `fill` (NaN for inputs: a kernel that reads the gap poisons its result)."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _rne(t):
    """fp32 -> bf16 bit patterns, round to nearest even (torch's CPU conversion)."""
    return _bits16(t.contiguous().to(torch.bfloat16))


RATIOS = {}


def _within(name, got, want, mag, factor, where, more=None):
    """|got - want| <= factor * u * mag (+ u * more), elementwise; keeps the largest error / bound ratio seen per quantity."""
    err = (got.to(F64) - want).abs()
    bound = factor * U * mag
    if more is not None:
        bound = bound + U * more
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if bool(torch.isfinite(got).all()) else math.inf
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    ok = err <= bound
    if not bool(ok.all()):
        i = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf).flatten()))
        raise AssertionError("%s %s: error / bound = %.3g at flat index %d (got %r, want %r, bound %.3e); %d of %d outside" % (
            name, where, worst, i, float(got.flatten()[i]), float(want.flatten()[i]), float(bound.flatten()[i]), int((~ok).sum()), ok.numel()))


def _ratio_only(name, got, want, bound):
    """A figure for the record (module docstring), no assertion."""
    err = (got.to(F64) - want).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio.max()))


def _report(what):
    print("\n[%s] largest error / bound so far: %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items()))))


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


# ---- CPU: the yardstick itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(63, 68), (257, 132)])
def test_references_agree_with_autograd_in_float64(M, C):
    """ref_bn_forward / ref_bn_backward / ref_colsum against torch.autograd on F.batch_norm(training=True) and F.relu in float64, to 1e-12
    relative to the magnitudes the bounds are built from (special channels included: the constant channel's dgamma is exactly 0)."""
    d = _data(M, C)
    x = d.x.to(F64).requires_grad_(True)
    gamma, beta = d.gamma.to(F64).requires_grad_(True), d.beta.to(F64).requires_grad_(True)
    rm, rv = d.rm.to(F64).clone(), d.rv.to(F64).clone()
    dy = d.dy.to(F64)
    with torch.enable_grad():
        pre = F.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS)
        y = F.relu(pre)
        y.backward(dy)
    f = ref_bn_forward(d.x, d.gamma, d.beta, EPS, MOMENTUM, 1, None, d.rm, d.rv)
    f0 = ref_bn_forward(d.x, d.gamma, d.beta, EPS, MOMENTUM, 0)
    b = ref_bn_backward(d.dy, d.x, f["y"], d.gamma, f["mu"], f["rstd"])

    def rel(got, want, mag):
        assert bool(((got - want).abs() <= 1e-12 * mag).all()), float(((got - want).abs() / mag.clamp_min(1e-300)).max())

    rel(f0["y"], pre.detach(), f0["y_mag"])
    rel(f["y"], y.detach(), f["y_mag"])
    rel(f["rm"], rm, f["rm_mag"])
    rel(f["rv"], rv, f["rv_mag"])
    rel(b["dx"], x.grad, b["dx_mag"])
    rel(b["dgamma"], gamma.grad, b["dgamma_mag"])
    rel(b["dbeta"], beta.grad, b["dbeta_mag"])
    assert float(b["dgamma"][d.const]) == 0.0 and float(b["dgamma_mag"][d.const]) == 0.0
    s, mag = ref_colsum(d.dy)
    rel(s, dy.sum(0), mag)
    # without the gate: the ReLU-free backward
    x.grad = gamma.grad = beta.grad = None
    with torch.enable_grad():
        F.batch_norm(x, None, None, gamma, beta, True, MOMENTUM, EPS).backward(dy)
    b = ref_bn_backward(d.dy, d.x, None, d.gamma, f["mu"], f["rstd"])
    rel(b["dx"], x.grad, b["dx_mag"])
    rel(b["dgamma"], gamma.grad, b["dgamma_mag"])
    rel(b["dbeta"], beta.grad, b["dbeta_mag"])


def test_chunk_counts_reach_the_reduction_rounds():
    """The shapes above are chosen for their chunk counts: 63 (two rounds of 32, the second clamped), 32 (one full round), 417 (14 rounds,
    fold not offered).  Recomputed from vidc_train_scratch_bytes and from the restatement above, so a retune of rows_for cannot silently
    drop the coverage."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    for M, C, _ in SHAPES + [(1, 8, 12)]:
        assert _lib_chunks(lib, M, C) == _chunks_for(M, C), (M, C)
    for (M, C, _), n in CHUNKS.items():
        assert _lib_chunks(lib, M, C) == n, (M, C)
    assert (_rows_for(2000, 4), _rows_for(1000, 68), _rows_for(20000, 8)) == (32, 32, 48)
    assert [_fold_offered(M, C) for M, C, _ in SHAPES] == [True] * 8 + [False]
    assert 417 > 13 * 32 and 63 % 32 != 0


# ---- GPU: BatchNorm forward --------------------------------------------------------------------------------------------------------------
def _scratch(lib, M, C):
    return torch.full((lib.vidc_train_scratch_bytes(M, C),), 0xFF, dtype=torch.uint8, device=DEV)      # (all-ones doubles are NaN)


def _run_forward(L, d, ld, relu, with_res, with_bf16):
    lib = L.lib()
    M, C = d.M, d.C
    ldx, ldy, ldr, _ = _strides(C, ld)
    x, y = _rows(d.x, ldx), torch.full((M, ldy), SENTINEL, device=DEV)
    res = _rows(d.res, ldr) if with_res else None
    gamma, beta, rm, rv = d.gamma.to(DEV), d.beta.to(DEV), d.rm.to(DEV), d.rv.to(DEV)
    mean, rstd = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    yb = torch.full((M, C), -1, dtype=torch.int16, device=DEV) if with_bf16 else None
    sc = _scratch(lib, M, C)
    if with_res:
        L.check(lib.vidc_bn_train_forward_add(L.ptr(x), L.ptr(y), M, C, ldx, ldy, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), EPS, MOMENTUM, relu,
                                              L.ptr(mean), L.ptr(rstd), L.ptr(yb), L.ptr(res), ldr, L.ptr(sc), L.current_stream()), "bn forward add")
    else:
        L.check(lib.vidc_bn_train_forward(L.ptr(x), L.ptr(y), M, C, ldx, ldy, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), EPS, MOMENTUM, relu,
                                          L.ptr(mean), L.ptr(rstd), L.ptr(yb), L.ptr(sc), L.current_stream()), "bn forward")
    torch.cuda.synchronize()
    return dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), rm=rm.cpu(), rv=rv.cpu(), **({"yb": yb.cpu()} if with_bf16 else {}))


def _check_forward(out, ref, C, where):
    _within("y", out["y"][:, :C], ref["y"], ref["y_mag"], 8, where)
    _within("save_mean", out["mean"], ref["mu"], ref["mu_mag"], 2, where)
    _within("save_rstd", out["rstd"], ref["rstd"], ref["rstd_mag"], 2, where)
    _within("running_mean", out["rm"], ref["rm"], ref["rm_mag"], 2, where)
    _within("running_var", out["rv"], ref["rv"], ref["rv_mag"], 2, where)
    assert bool((out["y"][:, C:] == SENTINEL).all()), "%s: the ld - C gap of y was written" % where
    if "yb" in out:
        assert torch.equal(out["yb"], _rne(out["y"][:, :C])), "%s: y_bf16 is not RNE(y) as dense rows of C" % where


def _both_folds(lib, run):
    """run() under vidc_train_bn_fold(0) and (1); the previous value is put back.  Returns the two results."""
    prev = lib.vidc_train_bn_fold(0)
    try:
        a = run()
        lib.vidc_train_bn_fold(1)
        b = run()
    finally:
        lib.vidc_train_bn_fold(prev)
    return a, b


def _assert_fold_identical(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), "%s: %s differs between vidc_train_bn_fold(0) and (1)" % (where, k)


@gpu
@pytest.mark.parametrize("M,C,ld", SHAPES, ids=_IDS)
def test_bn_forward(M, C, ld):
    """vidc_bn_train_forward / vidc_bn_train_forward_add: relu in {0, 1}, with and without a residual of its own stride, with and without
    the dense bf16 copy, separate and folded final reduction (bit-identical; for 20000 x 8 the switch must change nothing because the
    fold is not offered there).  y, save_mean, save_rstd and the running statistics against the float64 reference under the bounds of the
    module docstring; y_bf16 bit-equal to RNE of the fp32 y of the same call; the gap of y untouched."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    assert _lib_chunks(lib, M, C) == CHUNKS.get((M, C, ld), _chunks_for(M, C))
    d = _data(M, C)
    for relu in (0, 1):
        for with_res in (False, True):
            ref = ref_bn_forward(d.x, d.gamma, d.beta, EPS, MOMENTUM, relu, d.res if with_res else None, d.rm, d.rv)
            for with_bf16 in (False, True):
                where = "(%d, %d, %d) relu=%d res=%d bf16=%d" % (M, C, ld, relu, with_res, with_bf16)
                a, b = _both_folds(lib, lambda: _run_forward(L, d, ld, relu, with_res, with_bf16))
                _check_forward(a, ref, C, where + " fold=0")
                _check_forward(b, ref, C, where + " fold=1")
                _assert_fold_identical(a, b, where)
    _report("bn forward %s" % ((M, C, ld),))


@gpu
def test_bn_forward_single_row():
    """M = 1 (torch refuses it; the kernel's choice: unbiased = biased variance = 0): y == beta within the bound of y, everything finite,
    running_var == (1 - momentum) * old within 2u."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    d = _data(1, 8)
    ref = ref_bn_forward(d.x, d.gamma, d.beta, EPS, MOMENTUM, 0, None, d.rm, d.rv)
    assert float(ref["var"].abs().max()) == 0.0
    a, b = _both_folds(lib, lambda: _run_forward(L, d, 12, 0, False, True))
    for out, where in ((a, "M=1 fold=0"), (b, "M=1 fold=1")):
        assert all(bool(torch.isfinite(v.float()).all()) for k, v in out.items() if k not in ("y", "yb")) and bool(torch.isfinite(out["y"][:, :8]).all())
        _within("y (M=1)", out["y"][:, :8], d.beta.to(F64)[None], ref["y_mag"], 8, where)
        _within("running_var (M=1)", out["rv"], (1.0 - MOMENTUM) * d.rv.to(F64), d.rv.to(F64).abs(), 2, where)
        _check_forward(out, ref, 8, where)
    _assert_fold_identical(a, b, "M=1")
    _report("bn forward M=1")


# ---- GPU: BatchNorm backward -------------------------------------------------------------------------------------------------------------
def _backward_inputs(d):
    """save_mean / save_rstd: the float64 reference's, rounded to fp32 on the CPU (the backward is tested independently of the forward
    kernel); y_relu: the reference forward with ReLU, the `neg` channel forced to zeros of both signs (every gate closed)."""
    f = ref_bn_forward(d.x, d.gamma, d.beta, EPS, MOMENTUM, 1)
    y_relu = f["y"].float()
    if d.neg is not None:
        y_relu[:, d.neg] = 0.0
        y_relu[1::2, d.neg] = -0.0
    return f["mu"].float(), f["rstd"].float(), y_relu


def _run_backward(L, d, ld, mean, rstd, y_relu, with_dx, with_bf16, with_t):
    lib = L.lib()
    M, C = d.M, d.C
    Mp = (M + 63) // 64 * 64
    lddy, ldx, ldy, lddx = _strides(C, ld)
    dy, x = _rows(d.dy, lddy), _rows(d.x, ldx)
    y = _rows(y_relu, ldy) if y_relu is not None else None
    dx = torch.full((M, lddx), SENTINEL, device=DEV) if with_dx else None
    dxb = torch.full((M, C), -1, dtype=torch.int16, device=DEV) if with_bf16 else None
    dxt = torch.full((C, Mp), -1, dtype=torch.int16, device=DEV) if with_t else None          # 0xFFFF
    gamma, mean_d, rstd_d = d.gamma.to(DEV), mean.to(DEV), rstd.to(DEV)
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    sc = _scratch(lib, M, C)
    if with_t:
        L.check(lib.vidc_bn_train_backward_t(L.ptr(dy), L.ptr(x), L.ptr(y), L.ptr(dx), M, C, lddy, ldx, ldy, lddx, L.ptr(gamma), L.ptr(mean_d), L.ptr(rstd_d),
                                             L.ptr(dg), L.ptr(db), L.ptr(dxb), L.ptr(dxt), Mp, L.ptr(sc), L.current_stream()), "bn backward_t")
    else:
        L.check(lib.vidc_bn_train_backward(L.ptr(dy), L.ptr(x), L.ptr(y), L.ptr(dx), M, C, lddy, ldx, ldy, lddx, L.ptr(gamma), L.ptr(mean_d), L.ptr(rstd_d),
                                           L.ptr(dg), L.ptr(db), L.ptr(dxb), L.ptr(sc), L.current_stream()), "bn backward")
    torch.cuda.synchronize()
    out = dict(dgamma=dg.cpu(), dbeta=db.cpu())
    for k, v in (("dx", dx), ("dxb", dxb), ("dxt", dxt)):
        if v is not None:
            out[k] = v.cpu()
    return out


def _check_backward(out, ref, M, C, where, dx_of=None):
    """dx_of: the fp32 dx of the call with the same inputs that wrote one (for the dx == NULL form)."""
    _within("dgamma", out["dgamma"], ref["dgamma"], ref["dgamma_mag"], 4, where)
    _within("dbeta", out["dbeta"], ref["dbeta"], ref["dbeta_mag"], 2, where)
    if "dx" in out:
        _within("dx", out["dx"][:, :C], ref["dx"], ref["dx_mag"], 8, where, 2 * ref["dx_sum_mag"])
        _ratio_only("dx without the 2u term (not asserted)", out["dx"][:, :C], ref["dx"], 8 * U * ref["dx_mag"])
        assert bool((out["dx"][:, C:] == SENTINEL).all()), "%s: the gap of dx was written" % where
        dx_of = out["dx"][:, :C]
    want = _rne(dx_of)
    if "dxb" in out:
        assert torch.equal(out["dxb"], want), "%s: dx_bf16 is not RNE(dx) as dense rows of C" % where
    if "dxt" in out:
        assert torch.equal(out["dxt"][:, :M], want.t()), "%s: dx_bf16_t is not RNE(dx) transposed" % where
        assert bool((out["dxt"][:, M:] == 0).all()), "%s: the columns m >= M of dx_bf16_t are not 0x0000" % where


@gpu
@pytest.mark.parametrize("M,C,ld", SHAPES, ids=_IDS)
def test_bn_backward(M, C, ld):
    """vidc_bn_train_backward / vidc_bn_train_backward_t: with and without y_relu, with and without dx_bf16, with dx_bf16_t ([C][Mp] over a
    0xFFFF pre-fill, Mp = M rounded up to 64: RNE(dx) transposed, 0x0000 for m >= M), and the dx == NULL form with both bf16 outputs
    (bit-equal to RNE of the dx of the call that wrote one); all of it with the separate and the folded final reduction, bit-identical.
    dgamma, dbeta, dx against the float64 reference computed from the GIVEN save_mean / save_rstd."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    d = _data(M, C)
    mean, rstd, y_relu = _backward_inputs(d)
    for y_in in (None, y_relu):
        ref = ref_bn_backward(d.dy, d.x, y_in, d.gamma, mean, rstd)
        if y_in is not None and d.neg is not None:
            assert float(ref["dx_mag"][:, d.neg].max()) == 0.0      # closed gates: the bound is 0, the kernel must write exact zeros
        dx_seen = None
        for with_dx, with_bf16, with_t in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 1, 1)):
            where = "(%d, %d, %d) y_relu=%d dx=%d bf16=%d t=%d" % (M, C, ld, y_in is not None, with_dx, with_bf16, with_t)
            a, b = _both_folds(lib, lambda: _run_backward(L, d, ld, mean, rstd, y_in, with_dx, with_bf16, with_t))
            _check_backward(a, ref, M, C, where + " fold=0", dx_seen)
            _check_backward(b, ref, M, C, where + " fold=1", dx_seen)
            _assert_fold_identical(a, b, where)
            if with_dx and with_t:
                dx_seen = a["dx"][:, :C].contiguous()             # (the same kernel as the dx == NULL form)
    _report("bn backward %s" % ((M, C, ld),))


@gpu
@pytest.mark.parametrize("M,C,ld", SHAPES, ids=_IDS)
def test_colsum(M, C, ld):
    """vidc_colsum against the float64 column sums, 2u * S|.|; rows of stride ld > C (the dense shapes of the table also at C + 4)."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    d = _data(M, C)
    want, mag = ref_colsum(d.x)
    for stride in sorted({ld, max(ld, C + 4)}):
        a = _rows(d.x, stride)
        out = torch.full((C,), float("nan"), device=DEV)
        sc = _scratch(lib, M, C)
        L.check(lib.vidc_colsum(L.ptr(a), M, C, stride, L.ptr(out), L.ptr(sc), L.current_stream()), "colsum")
        torch.cuda.synchronize()
        _within("colsum", out.cpu(), want, mag, 2, "(%d, %d, %d)" % (M, C, stride))
    _report("colsum %s" % ((M, C, ld),))


# ---- GPU: exact kernels (torch.equal against fp32 torch on the CPU) ----------------------------------------------------------------------
@gpu
def test_add_rows_exact():
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    M, C, lda, ldb, ldy = 100, 12, 16, 20, 24                     # 300 threads: two workgroups
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    ad, bd = _rows(a, lda), _rows(b, ldb)
    for relu in (0, 1):
        want = (a + b).clamp_min(0.0) if relu else a + b
        y = torch.full((M, ldy), SENTINEL, device=DEV)
        L.check(lib.vidc_add_rows(L.ptr(ad), L.ptr(bd), L.ptr(y), M, C, lda, ldb, ldy, relu, L.current_stream()), "add_rows")
        y2, yb = torch.full((M, ldy), SENTINEL, device=DEV), torch.full((M, C), -1, dtype=torch.int16, device=DEV)
        L.check(lib.vidc_add_rows_bf16(L.ptr(ad), L.ptr(bd), L.ptr(y2), M, C, lda, ldb, ldy, relu, L.ptr(yb), L.current_stream()), "add_rows_bf16")
        torch.cuda.synchronize()
        for t in (y.cpu(), y2.cpu()):
            assert torch.equal(t[:, :C], want) and bool((t[:, C:] == SENTINEL).all()), relu
        assert torch.equal(yb.cpu(), _rne(want)), relu


@gpu
def test_relu_backward_exact():
    """dx (=|+=) dy * (y > 0) with a y that holds exact zeros of both signs; y == NULL: plain copy / accumulate."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    M, C, lddy, ldy, lddx = 100, 12, 16, 20, 24
    g = torch.Generator().manual_seed(4)
    dy, y, old = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    y[::3] = 0.0
    y[1::3, ::2] = -0.0
    dyd, yd = _rows(dy, lddy), _rows(y, ldy)
    for y_in in (None, yd):
        gated = dy if y_in is None else torch.where(y > 0, dy, torch.zeros_like(dy))
        for accumulate in (0, 1):
            dx = _rows(old, lddx, SENTINEL)
            L.check(lib.vidc_relu_backward(L.ptr(dyd), L.ptr(y_in), L.ptr(dx), M, C, lddy, ldy, lddx, accumulate, L.current_stream()), "relu_backward")
            torch.cuda.synchronize()
            got = dx.cpu()
            assert torch.equal(got[:, :C], gated + old if accumulate else gated), (y_in is not None, accumulate)
            assert bool((got[:, C:] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("stride,Ho,Wo,H,W", [(1, 5, 7, 5, 7), (2, 5, 7, 9, 14), (2, 5, 7, 10, 13)])
def test_zero_stuff_exact(stride, Ho, Wo, H, W):
    """z[b, oy*s, ox*s] = dy[b, oy, ox], zero elsewhere, with lddy > C; (H, W) = (2Ho - 1, 2Wo) and (2Ho, 2Wo - 1): the last row / column is a
    source in one dimension and not in the other."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    B, C, lddy = 2, 12, 20
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(B * Ho * Wo, C, generator=g)
    z = torch.full((B, H, W, C), SENTINEL, device=DEV)
    dyd = _rows(dy, lddy)
    L.check(lib.vidc_zero_stuff(L.ptr(dyd), L.ptr(z), B, Ho, Wo, C, lddy, stride, H, W, L.current_stream()), "zero_stuff")
    torch.cuda.synchronize()
    want = torch.zeros(B, H, W, C)
    want[:, ::stride, ::stride][:, :Ho, :Wo] = dy.view(B, Ho, Wo, C)
    assert torch.equal(z.cpu(), want)


@gpu
@pytest.mark.parametrize("taps", [1, 9])
def test_wgrad_permute_exact(taps):
    """dw_oihw[co][ci][tap] = tmp[co][tap * Cin + ci], Cout and Cin multiples of nothing."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    Cout, Cin = 5, 7
    tmp = torch.randn(Cout, taps * Cin, generator=torch.Generator().manual_seed(6))
    dw = torch.full((Cout, Cin, taps), SENTINEL, device=DEV)
    tmpd = tmp.to(DEV)
    L.check(lib.vidc_wgrad_permute(L.ptr(tmpd), L.ptr(dw), Cout, Cin, taps, L.current_stream()), "wgrad_permute")
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), tmp.view(Cout, taps, Cin).permute(0, 2, 1).contiguous())


@gpu
@pytest.mark.parametrize("M,C", [(65, 8), (130, 72), (64, 64)])
def test_transpose_bf16_exact(M, C):
    """Dense bf16 rows [M][C] -> [C][Mp], zeros for m >= M over a 0xFFFF pre-fill."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    Mp = (M + 63) // 64 * 64
    x = _rne(torch.randn(M, C, generator=torch.Generator().manual_seed(7)))
    xd, xt = x.to(DEV), torch.full((C, Mp), -1, dtype=torch.int16, device=DEV)
    L.check(lib.vidc_transpose_bf16(L.ptr(xd), L.ptr(xt), M, C, Mp, L.current_stream()), "transpose_bf16")
    torch.cuda.synchronize()
    got = xt.cpu()
    assert torch.equal(got[:, :M], x.t()) and bool((got[:, M:] == 0).all())


_TIES = [1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8, -(1.0 + 3 * 2.0 ** -8), -(1.0 + 2.0 ** -8), 2.0 ** -126, 0.0, -0.0]      # RNE ties: up to even (first: a tail that truncates shows), down to even


@gpu
def test_cast_bf16_exact():
    """fp32 rows of stride ldx > C -> dense bf16 rows, round to nearest even (ties included)."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    rows, C, ldx = 70, 24, 28                                     # 210 threads
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(8))
    x[0, :len(_TIES)] = torch.tensor(_TIES)
    xd, y = _rows(x, ldx), torch.full((rows, C), -1, dtype=torch.int16, device=DEV)
    L.check(lib.vidc_cast_bf16(L.ptr(xd), L.ptr(y), rows, C, ldx, L.current_stream()), "cast_bf16")
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), _rne(x))


@gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
def test_grad_narrow_widen_exact(n):
    """vidc_grad_narrow_bf16 bit-equal to .to(torch.bfloat16) (NaN: any NaN pattern), vidc_grad_widen_bf16 bit-equal to .float(); the 8-wide body (i + 8 <= n) and the
    scalar tail round the same values identically; +-inf and the canonical quiet NaN come back as inf and NaN (a diverged rank stays
    visible after the bucket sum); nothing is written past n."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    special = _TIES[:4] + [math.inf, -math.inf, math.nan]
    base = torch.randn(2055, generator=torch.Generator().manual_seed(9)) * 3
    base[:7] = torch.tensor(special)
    x = base[:n].clone()
    body = n // 8 * 8
    if 0 < body < n:                                              # the tail repeats the first values of the body
        x[body:] = x[:n - body]
    pad = 16
    xd = x.to(DEV)
    nb = torch.full((n + pad,), -1, dtype=torch.int16, device=DEV)
    L.check(lib.vidc_grad_narrow_bf16(L.ptr(xd), L.ptr(nb), n, L.current_stream()), "grad_narrow")
    wide = torch.full((n + pad,), SENTINEL, device=DEV)
    L.check(lib.vidc_grad_widen_bf16(L.ptr(nb), L.ptr(wide), n, L.current_stream()), "grad_widen")
    torch.cuda.synchronize()
    got, back = nb.cpu(), wide.cpu()
    want, nan = _rne(x), torch.isnan(x)
    # (torch's CPU conversion encodes NaN as 0x7FC0 in its scalar path and as 0xFFFF in its vector path: any NaN pattern is accepted there)
    assert torch.equal(got[:n][~nan], want[~nan]) and bool((got[n:] == -1).all())
    assert bool(((got[:n][nan].to(torch.int32) & 0x7FFF) > 0x7F80).all()), "NaN narrowed to something that is no NaN"
    if 0 < body < n:
        assert torch.equal(got[body:n], got[:n - body]), "tail and body round differently"
    assert _same_bits(back[:n], got[:n].view(torch.bfloat16).float()) and bool((back[n:] == SENTINEL).all())
    assert torch.equal(torch.isnan(back[:n]), nan) and torch.equal(back[:n][~nan], x[~nan].to(torch.bfloat16).float())
    for i, v in enumerate(special[:n]):
        assert (math.isnan(float(back[i])) if math.isnan(v) else float(back[i]) == float(torch.tensor(v).to(torch.bfloat16))), (i, v)
    if n > 6:
        assert float(back[4]) == math.inf and float(back[5]) == -math.inf and math.isnan(float(back[6]))


# ---- GPU: the bits of every row kernel, as recorded before the kernels shared their bodies ----------------------------------------------------
BITS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_rows_bits.json")
BITS_SHAPE = (70, 68, 72)         # a ragged last channel block (68 = 64 + 4), a ragged last 64-row tile (70 = 64 + 6) and a ragged 16-row lane


def _sha(*tensors):
    """SHA-256 of the raw bytes of the tensors, one after the other (None: skipped)."""
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _sha_dict(out):
    return _sha(*[out[k] for k in sorted(out)])


def _chunk_table(x, rows):
    """The per-channel partial sums of x [M][C] in chan_partial_kernel's layout, [chunk][sum x | sum x^2][C] in float64 for chunks of `rows`
    rows, each chunk added row by row on the CPU (a fixed order: the same table everywhere)."""
    M, C = x.shape
    t = torch.zeros((M + rows - 1) // rows, 2, C, dtype=F64)
    for r in range(M):
        v = x[r].to(F64)
        t[r // rows, 0] += v
        t[r // rows, 1] += v * v
    return t


def _bits_bn(L, bits):
    lib = L.lib()
    M, C, ld = BITS_SHAPE
    d = _data(M, C)
    for with_res in (0, 1):
        for relu in (0, 1):
            for with_bf16 in (0, 1):
                a, b = _both_folds(lib, lambda: _run_forward(L, d, ld, relu, bool(with_res), bool(with_bf16)))
                for fold, out in ((0, a), (1, b)):
                    bits["bn_forward/res%d_relu%d_bf16%d_fold%d" % (with_res, relu, with_bf16, fold)] = _sha_dict(out)
    # vidc_bn_train_forward_stats: the chunk sums come from the conv that wrote x, one pair of rows per 32 output rows
    ldx, ldy, ldr, _ = _strides(C, ld)
    stats = _chunk_table(d.x, 32).to(DEV)
    for with_res, relu, with_bf16 in ((0, 0, 0), (1, 1, 1)):
        x, y = _rows(d.x, ldx), torch.full((M, ldy), SENTINEL, device=DEV)
        res = _rows(d.res, ldr) if with_res else None
        gamma, beta, rm, rv = d.gamma.to(DEV), d.beta.to(DEV), d.rm.to(DEV), d.rv.to(DEV)
        mean, rstd = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        yb = torch.full((M, C), -1, dtype=torch.int16, device=DEV) if with_bf16 else None
        sc = _scratch(lib, M, C)
        L.check(lib.vidc_bn_train_forward_stats(L.ptr(x), L.ptr(y), M, C, ldx, ldy, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), EPS, MOMENTUM, relu,
                                                L.ptr(mean), L.ptr(rstd), L.ptr(yb), L.ptr(res), ldr, L.ptr(stats), L.ptr(sc), L.current_stream()),
                "bn forward stats")
        torch.cuda.synchronize()
        bits["bn_forward_stats/res%d_relu%d_bf16%d" % (with_res, relu, with_bf16)] = _sha(y, yb, mean, rstd, rm, rv)
    mean, rstd, y_relu = _backward_inputs(d)
    for y_in in (None, y_relu):
        for with_dx, with_bf16, with_t in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)):
            a, b = _both_folds(lib, lambda: _run_backward(L, d, ld, mean, rstd, y_in, with_dx, with_bf16, with_t))
            for fold, out in ((0, a), (1, b)):
                bits["bn_backward/y%d_dx%d_bf16%d_t%d_fold%d" % (y_in is not None, with_dx, with_bf16, with_t, fold)] = _sha_dict(out)


def _bits_rows(L, bits):
    lib = L.lib()
    M, C, ld = 5, 12, 16
    g = torch.Generator().manual_seed(21)
    a, b, old = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    b[::2, ::3] = 0.0
    b[1::2, 1::3] = -0.0
    ad, bd = _rows(a, ld), _rows(b, ld)
    out = torch.full((C,), float("nan"), device=DEV)
    sc = _scratch(lib, M, C)
    L.check(lib.vidc_colsum(L.ptr(ad), M, C, ld, L.ptr(out), L.ptr(sc), L.current_stream()), "colsum")
    bits["colsum"] = _sha(out)
    for relu in (0, 1):
        for with_bf16 in (0, 1):
            y = torch.full((M, ld), SENTINEL, device=DEV)
            yb = torch.full((M, C), -1, dtype=torch.int16, device=DEV) if with_bf16 else None
            L.check(lib.vidc_add_rows_bf16(L.ptr(ad), L.ptr(bd), L.ptr(y), M, C, ld, ld, ld, relu, L.ptr(yb), L.current_stream()), "add_rows_bf16")
            bits["add_rows/relu%d_bf16%d" % (relu, with_bf16)] = _sha(y, yb)
    for y_in in (None, bd):
        for accumulate in (0, 1):
            dx = _rows(old, ld, SENTINEL)
            L.check(lib.vidc_relu_backward(L.ptr(ad), L.ptr(y_in), L.ptr(dx), M, C, ld, ld, ld, accumulate, L.current_stream()), "relu_backward")
            bits["relu_backward/y%d_acc%d" % (y_in is not None, accumulate)] = _sha(dx)
    x8 = torch.randn(M, 8, generator=g)
    x8[0, :len(_TIES)] = torch.tensor(_TIES)
    xd, y = _rows(x8, ld), torch.full((M, 8), -1, dtype=torch.int16, device=DEV)
    L.check(lib.vidc_cast_bf16(L.ptr(xd), L.ptr(y), M, 8, ld, L.current_stream()), "cast_bf16")
    bits["cast_bf16"] = _sha(y)


def _bits_pool_upsample(L, bits):
    """Both launch forms of each: four channels per thread (aligned, strides multiples of 4) and one (forced by lddx = C + 1)."""
    lib = L.lib()
    B, C = 2, 8
    g = torch.Generator().manual_seed(22)
    for H, W in ((5, 7), (6, 4), (1, 1)):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = torch.randint(0, 4, (B, H, W, C), generator=g).float().to(DEV)          # small integers: ties in most windows
        dy = torch.randn(B, Ho, Wo, C, generator=g).to(DEV)
        for form, lddx in (("wide", C), ("scalar", C + 1)):
            dx = torch.full((B, H, W, lddx), SENTINEL, device=DEV)
            L.check(lib.vidc_maxpool3x3s2_backward(L.ptr(x), L.ptr(dy), L.ptr(dx), B, H, W, C, C, C, lddx, L.current_stream()), "maxpool_bwd")
            bits["maxpool_backward/%dx%d_%s" % (H, W, form)] = _sha(dx[..., :C])
            assert bool((dx[..., C:] == SENTINEL).all())
    for h, w, H, W in ((3, 4, 7, 9), (1, 1, 3, 3), (4, 4, 4, 4)):                    # the second has scale 0, the third is the identity
        dy = torch.randn(B, H, W, C, generator=g).to(DEV)
        for form, lddx in (("wide", C), ("scalar", C + 1)):
            dx = torch.full((B, h, w, lddx), SENTINEL, device=DEV)
            L.check(lib.vidc_upsample_bilinear_ac_backward(L.ptr(dy), L.ptr(dx), B, h, w, C, C, lddx, H, W, L.current_stream()), "upsample_bwd")
            bits["upsample_backward/%dx%d_to_%dx%d_%s" % (h, w, H, W, form)] = _sha(dx[..., :C])
            assert bool((dx[..., C:] == SENTINEL).all())


def _bits_im2col(L, bits):
    """The whole xt buffer over a constant pre-fill: the padding columns m >= M and every byte the kernel leaves alone are pinned too."""
    lib = L.lib()
    B, H, W, stride, pad = 2, 5, 6, 2, 1
    g = torch.Generator().manual_seed(23)
    for C, ldx in ((8, 12), (6, 8)):                                                 # the 64 x 64 kernel; the 32 x 32 one (C % 4 != 0)
        x = _rows(torch.randn(B * H * W, C, generator=g), ldx)
        for k in (3, 1):
            for dil in (1, 2):
                Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
                M = B * Ho * Wo
                for split in (0, 1, 2, 4, 5, 6):
                    Mp = (M + 63) // 64 * 64 if split & 3 == 2 else (M + 31) // 32 * 32
                    xt = torch.full((k * k * C, Mp), SENTINEL, device=DEV)
                    if dil == 1:
                        L.check(lib.vidc_im2col_transposed(L.ptr(x), L.ptr(xt), B, H, W, C, ldx, Ho, Wo, k, k, stride, pad, Mp, split, L.current_stream()),
                                "im2col_transposed")
                    else:
                        L.check(lib.vidc_im2col_transposed_dilated(L.ptr(x), L.ptr(xt), B, H, W, C, ldx, Ho, Wo, k, k, stride, pad, dil, Mp, split,
                                                                   L.current_stream()), "im2col_transposed_dilated")
                    bits["im2col/C%d_k%d_dil%d_split%d" % (C, k, dil, split)] = _sha(xt)
    for C in (8, 72):
        xb = _rne(torch.randn(B * H * W, C, generator=g)).to(DEV)
        for k in (3, 1):
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            Mp = (B * Ho * Wo + 63) // 64 * 64
            xt = torch.full((k * k * C, Mp), -1, dtype=torch.int16, device=DEV)
            L.check(lib.vidc_im2col_transposed_bf16(L.ptr(xb), L.ptr(xt), B, H, W, C, Ho, Wo, k, k, stride, pad, Mp, L.current_stream()), "im2col_transposed_bf16")
            bits["im2col_bf16/C%d_k%d" % (C, k)] = _sha(xt)
        xt = torch.full((C, 64), -1, dtype=torch.int16, device=DEV)
        L.check(lib.vidc_transpose_bf16(L.ptr(xb), L.ptr(xt), B * H * W, C, 64, L.current_stream()), "transpose_bf16")
        bits["transpose_bf16/C%d" % C] = _sha(xt)


def _train_rows_bits():
    """name -> SHA-256 of the raw output bytes of every kernel of csrc/train.hip that is built from the shared row helpers and bodies, each at the
    smallest shape that reaches all of its branches.  Inputs are seeded CPU tensors."""
    from vi_depth_completion_amd import _lib as L
    bits = {}
    _bits_bn(L, bits)
    _bits_rows(L, bits)
    _bits_pool_upsample(L, bits)
    _bits_im2col(L, bits)
    return bits


@gpu
def test_output_bits_are_those_recorded_before_the_kernels_shared_their_bodies():
    """tests/golden/train_rows_bits.json was recorded on an MI355X from the library as it was when the BatchNorm apply and backward kernels, the
    max-pool and upsampling backward kernels and the im2col kernels each had two or three copies of their body: sharing one body per map, and the
    row-quad helpers of csrc/train_rows.h, changed no output bit (and no later change to them may, unless it says so)."""
    got = _train_rows_bits()
    with open(BITS_JSON) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    assert not [k for k in want if got[k] != want[k]], [k for k in want if got[k] != want[k]]
    for k in want:                                                                   # the launch forms of one map wrote the same bytes
        if k.endswith("_fold1"):
            assert want[k] == want[k[:-1] + "0"], k
        if k.endswith("_scalar"):
            assert want[k] == want[k[:-len("scalar")] + "wide"], k
