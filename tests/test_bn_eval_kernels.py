"""The two entries of the frozen (eval-mode) BatchNorm, vidc_bn_eval_forward_add and vidc_bn_eval_backward (csrc/train.hip), through the C ABI.

Built like tests/test_train_kernels.py (whose row helpers are imported): float64 references that read only the kernel's fp32 inputs, a
SENTINEL-filled ld - C gap in every output row, NaN in the gap of every input row, outputs inside guarded buffers (SENTINEL rows in front of
and behind the rows the kernel may write), a different row stride per tensor, x read in place as a channel slice of a wider tensor.  Shapes
(M, C, ld), six of that file's: the smallest legal one, a row past the 16 row-lanes, a partial second channel block, three channel blocks, 63
chunks with a clamped second round of the final reduction, 417 chunks.

Special channels (every shape has all three): `gz` with gamma = 0; `vz` with running_var = 0 (rstd = eps^-1/2 = 316.2, finite); `cn` with
x = 100 + 0.1 n and running_mean = 100.03 (|running_mean| 1000 times the spread of x: x - running_mean cancels three digits).

Bounds are elementwise, built from the reference's float64 magnitudes only, u = 2^-24.  A factor is the number of fp32 roundings on the worst
term plus one -- the headroom for the products of roundings, (1 + u)^n - 1 < (n + 1) u, and the fp64 accumulation -- which is how the header
of tests/test_train_kernels.py arrives at its factors (y there: 7 roundings, 8u).  Reading the kernels:

  y       7u (|x a| + |mu a| + |beta| + |res|)   a = fl(fl(rstd) * gamma): 2; fl(mu * a): 3 on |mu a|; beta - .: 4; x * a + bb (fused or not): 5;
                                                 + res: 6.  One fewer than the train-mode y: running_mean is an input, not a rounded fp64 mean.
                                                 The arithmetic is bn_apply_row's, so the FORM is the train-mode one.
  dx      4u |gamma rstd g'|                     fl(rstd): 1; fl(gamma * rstd): 2; fl(g' * gs): 3
  dgamma  5u S |g' xh|                           xh = fl(fl(x - mu) * fl(rstd)): 3 (x and mu are inputs: the difference has ONE relative rounding
                                                 however much it cancels); products and sums in fp64; the final rounding: 4
  dbeta   2u S |g'|                              fp64 sum, one rounding

Measured error / bound ratios on MI355X: profiles/EXPERIMENTS.md (each GPU test prints the largest it has seen).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_train_kernels import DEV, EPS, F64, SENTINEL, U, _chunks_for, _lib_chunks, _rows, _same_bits, _scratch  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(2, 4, 8), (17, 8, 12), (63, 68, 72), (257, 132, 160), (2000, 68, 100), (20000, 8, 8)]
CHUNKS = {(2000, 68): 63, (20000, 8): 417}
_IDS = ["%dx%d_ld%d" % s for s in SHAPES]
GUARD = 3                      # SENTINEL rows in front of and behind every output
K_Y, K_DX, K_DGAMMA, K_DBETA = 7, 4, 5, 2


# ---- float64 references -----------------------------------------------------------------------------------------------------------------
def ref_forward(x, gamma, beta, rm, rv, eps, relu, res=None):
    """nn.BatchNorm2d in eval() mode over the rows of x [M][C] (+ residual, + ReLU) and the magnitude the bound of y multiplies."""
    x, gamma, beta, rm, rv = (t.to(F64) for t in (x, gamma, beta, rm, rv))
    rstd = 1.0 / torch.sqrt(rv + eps)
    a = rstd * gamma
    y = x * a + (beta - rm * a)
    mag = (x * a).abs() + (rm * a).abs() + beta.abs()
    if res is not None:
        y = y + res.to(F64)
        mag = mag + res.to(F64).abs()
    pre = y
    if relu:
        y = y.clamp_min(0.0)
    return dict(y=y, pre=pre, y_mag=mag, rstd=rstd)


def ref_backward(dy, x, y_relu, gamma, rm, rv, eps):
    """g' = dy * (y_relu > 0); dx = g' gamma rstd; dgamma = S g' xh, xh = (x - running_mean) rstd; dbeta = S g'."""
    dy, x, gamma, rm, rv = (t.to(F64) for t in (dy, x, gamma, rm, rv))
    rstd = 1.0 / torch.sqrt(rv + eps)
    g = dy if y_relu is None else dy * (y_relu > 0).to(F64)
    xh = (x - rm) * rstd
    dx = g * gamma * rstd
    return dict(dx=dx, dgamma=(g * xh).sum(0), dbeta=g.sum(0), dx_mag=dx.abs(), dgamma_mag=(g * xh).abs().sum(0), dbeta_mag=g.abs().sum(0))


# ---- data -------------------------------------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, M, C):
        g = torch.Generator().manual_seed(7000 * M + C)
        self.M, self.C = M, C
        self.gz, self.vz, self.cn = 1, C - 2, C - 1
        x = torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + torch.randn(C, generator=g)
        x[:, self.cn] = 100.0 + 0.1 * torch.randn(M, generator=g)
        self.x = x
        self.dy = torch.randn(M, C, generator=g)
        self.res = torch.randn(M, C, generator=g)
        self.gamma = torch.rand(C, generator=g) + 0.5
        self.beta = torch.randn(C, generator=g) * 0.2
        self.rm = torch.randn(C, generator=g) * 0.5
        self.rv = torch.rand(C, generator=g) + 0.5
        self.gamma[self.gz] = 0.0
        self.rv[self.vz] = 0.0
        self.rm[self.cn] = 100.03
        # y_relu of the backward: the reference's ReLU output in fp32; channel 0 holds exact zeros of both signs in two rows of three
        y = ref_forward(self.x, self.gamma, self.beta, self.rm, self.rv, EPS, 1)["y"].float()
        y[::3, 0] = 0.0
        y[1::3, 0] = -0.0
        self.y_relu = y


_DATA = {}


def _data(M, C):
    if (M, C) not in _DATA:
        _DATA[(M, C)] = _Data(M, C)
    return _DATA[(M, C)]


def _strides(C, ld):
    """Four different row strides from ld on; the dense shape of the table stays dense for every tensor."""
    return (C,) * 4 if ld == C else (ld, ld + 4, ld + 8, ld + 12)


def _guarded(M, ld):
    """(buffer, rows): a SENTINEL-filled [GUARD + M + GUARD][ld] device buffer and the view of its M middle rows (16-byte aligned: ld % 4 == 0)."""
    buf = torch.full((M + 2 * GUARD, ld), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + M]


def _untouched(buf, C, where):
    """The guard rows and the ld - C gap of the rows in between still hold SENTINEL."""
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), "%s: written outside the M rows" % where
    assert bool((b[GUARD:-GUARD, C:] == SENTINEL).all()), "%s: the ld - C gap was written" % where


def _slice_of_wider(t, ld):
    """t [M][C] as channels 4..4+C of a [M][ld + 8] device tensor whose other channels are NaN: the view has row stride ld + 8 and starts 16
    bytes into the row (x read in place as a channel slice)."""
    wide = torch.full((t.shape[0], ld + 8), float("nan"))
    wide[:, 4:4 + t.shape[1]] = t
    wide = wide.to(DEV)
    return wide, wide[:, 4:4 + t.shape[1]], ld + 8


RATIOS = {}


def _within(name, got, want, mag, factor, where):
    err = (got.to(F64) - want).abs()
    bound = factor * U * mag
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(ratio.max()) if bool(torch.isfinite(got).all()) else math.inf
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    print("  %-8s %-46s error / bound %.3f" % (name, where, worst))
    if not worst <= 1.0:
        i = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf).flatten()))
        raise AssertionError("%s %s: error / bound = %.3g at flat index %d (got %r, want %r, bound %.3e)" % (
            name, where, worst, i, float(got.flatten()[i]), float(want.flatten()[i]), float(bound.flatten()[i])))


def _report(what):
    print("\n[%s] largest error / bound so far: %s" % (what, ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items()))))


# ---- CPU: the yardstick itself, and the host refusals ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(63, 68), (257, 132)])
def test_references_agree_with_autograd_in_float64(M, C):
    """ref_forward / ref_backward against torch.autograd on F.batch_norm(training=False) + residual + ReLU in float64, to 1e-12 of the
    magnitudes the bounds are built from; the special channels behave as designed."""
    d = _data(M, C)
    x, res = d.x.to(F64).requires_grad_(True), d.res.to(F64).requires_grad_(True)
    gamma, beta = d.gamma.to(F64).requires_grad_(True), d.beta.to(F64).requires_grad_(True)
    rm, rv = d.rm.to(F64).clone(), d.rv.to(F64).clone()

    def rel(got, want, mag):
        assert bool(((got - want).abs() <= 1e-12 * mag).all()), float(((got - want).abs() / mag.clamp_min(1e-300)).max())

    with torch.enable_grad():
        pre = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, EPS) + res
        y = F.relu(pre)
        y.backward(d.dy.to(F64))
    assert torch.equal(rm, d.rm.to(F64)) and torch.equal(rv, d.rv.to(F64))
    f = ref_forward(d.x, d.gamma, d.beta, d.rm, d.rv, EPS, 1, d.res)
    rel(f["pre"], pre.detach(), f["y_mag"])
    rel(f["y"], y.detach(), f["y_mag"])
    b = ref_backward(d.dy, d.x, f["y"], d.gamma, d.rm, d.rv, EPS)
    rel(b["dx"], x.grad, b["dx_mag"])
    rel(b["dgamma"], gamma.grad, b["dgamma_mag"])
    rel(b["dbeta"], beta.grad, b["dbeta_mag"])
    rel(b["dbeta"], res.grad.sum(0), b["dbeta_mag"])                 # (the residual's gradient is g' itself)
    x.grad = gamma.grad = beta.grad = None
    with torch.enable_grad():
        F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, EPS).backward(d.dy.to(F64))
    b = ref_backward(d.dy, d.x, None, d.gamma, d.rm, d.rv, EPS)
    rel(b["dx"], x.grad, b["dx_mag"])
    rel(b["dgamma"], gamma.grad, b["dgamma_mag"])
    rel(b["dbeta"], beta.grad, b["dbeta_mag"])
    assert float(b["dx"][:, d.gz].abs().max()) == 0.0 and float(b["dx_mag"][:, d.gz].max()) == 0.0      # gamma = 0: dx is exactly 0
    assert abs(float(f["rstd"][d.vz]) - EPS ** -0.5) < 1e-9 and math.isfinite(float(b["dgamma"][d.vz]))
    assert float((d.x[:, d.cn].to(F64) - 100.03).abs().max()) < 1.0 < 0.01 * float(d.rm[d.cn])


def test_data_reaches_the_reduction_rounds():
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    for M, C, _ in SHAPES:
        assert _lib_chunks(lib, M, C) == CHUNKS.get((M, C), _chunks_for(M, C)), (M, C)
    d = _data(63, 68)
    gate = d.y_relu > 0
    assert 0.2 < float(gate.float().mean()) < 0.8 and not bool(gate[::3, 0].any()) and not bool(gate[1::3, 0].any())


def test_host_refusals():
    """VIDC_REQUIRE refuses before anything is launched (so no GPU is needed): the shapes the train-mode entries refuse, and the pointer rules
    of the backward's optional parts.  The pointers are never dereferenced."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    p = 4096
    NULL, SHAPE = -1, -2

    def fwd(M=8, C=8, ldx=8, ldy=8, ldr=8, x=p, y=p, gamma=p, beta=p, rm=p, rv=p, res=p):
        return lib.vidc_bn_eval_forward_add(x, y, M, C, ldx, ldy, gamma, beta, rm, rv, EPS, 1, res, ldr, None)

    for kw in (dict(x=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(rm=None), dict(rv=None)):
        assert fwd(**kw) == NULL, kw
    for kw in (dict(M=0), dict(C=0), dict(C=6), dict(ldx=4), dict(ldy=4), dict(ldx=10), dict(ldy=10), dict(ldr=4), dict(ldr=10)):
        assert fwd(**kw) == SHAPE, kw
    assert b"vidc_bn_eval_forward_add" in lib.vidc_last_error()

    def bwd(M=8, C=8, lddy=8, ldx=8, ldy=8, lddx=8, dy=p, x=p, y=p, dx=p, gamma=p, rm=p, rv=p, dg=p, db=p, sc=p):
        return lib.vidc_bn_eval_backward(dy, x, y, dx, M, C, lddy, ldx, ldy, lddx, gamma, rm, rv, EPS, dg, db, sc, None)

    for kw in (dict(dy=None), dict(rm=None), dict(rv=None), dict(dg=None), dict(db=None), dict(x=None), dict(sc=None), dict(gamma=None),
               dict(dx=None, dg=None, db=None)):
        assert bwd(**kw) == NULL, kw
    for kw in (dict(M=0), dict(C=0), dict(C=6), dict(lddy=4), dict(lddy=10), dict(ldx=10), dict(ldy=10), dict(lddx=10), dict(lddx=4)):
        assert bwd(**kw) == SHAPE, kw
    assert b"vidc_bn_eval_backward" in lib.vidc_last_error()


# ---- GPU: forward ----------------------------------------------------------------------------------------------------------------------
def _stats(d):
    return [t.to(DEV) for t in (d.gamma, d.beta, d.rm, d.rv)]


@gpu
@pytest.mark.parametrize("M,C,ld", SHAPES, ids=_IDS)
def test_bn_eval_forward(M, C, ld):
    """relu in {0, 1}, with and without a residual of its own stride, x dense-strided and as a channel slice of a wider tensor: y within
    7u (|x a| + |mu a| + |beta| + |res|) of the float64 reference everywhere (special channels included), the gap and the guard rows of y and all
    four per-channel vectors bit-unchanged, the slice form bit-equal to the strided one."""
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    d = _data(M, C)
    ldx, ldy, ldr, _ = _strides(C, ld)
    stats = _stats(d)
    before = [t.clone() for t in stats]
    gamma, beta, rm, rv = stats
    res_d = _rows(d.res, ldr)
    wide, x_slice, ld_slice = _slice_of_wider(d.x, ld)
    for relu in (0, 1):
        for with_res in (False, True):
            ref = ref_forward(d.x, d.gamma, d.beta, d.rm, d.rv, EPS, relu, d.res if with_res else None)
            outs = []
            for form, (x, lx) in (("strided", (_rows(d.x, ldx), ldx)), ("slice", (x_slice, ld_slice))):
                where = "(%d, %d, %d) relu=%d res=%d x=%s" % (M, C, ld, relu, with_res, form)
                buf, y = _guarded(M, ldy)
                L.check(lib.vidc_bn_eval_forward_add(L.ptr(x), L.ptr(y), M, C, lx, ldy, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), EPS, relu,
                                                     L.ptr(res_d) if with_res else None, ldr if with_res else 0, L.current_stream()), "bn eval forward")
                torch.cuda.synchronize()
                got = y.cpu()[:, :C]
                _within("y", got, ref["y"], ref["y_mag"], K_Y, where)
                _untouched(buf, C, where)
                outs.append(got)
            assert _same_bits(outs[0], outs[1]), "x as a channel slice gives other bits"
    assert bool(torch.isfinite(outs[0][:, d.vz]).all())
    for t, b in zip(stats, before):
        assert _same_bits(t.cpu(), b.cpu()), "a per-channel vector (gamma, beta, running_mean, running_var) was written"
    _report("bn eval forward %s" % ((M, C, ld),))


# ---- GPU: backward ---------------------------------------------------------------------------------------------------------------------
def _launch_backward(L, d, ld, y_relu, with_dx, with_sums, stream=None, with_x=True):
    """Enqueue one call (buffers of its own) and return what _collect_backward reads once the device is idle."""
    lib = L.lib()
    M, C = d.M, d.C
    lddy, ldx, ldy, lddx = _strides(C, ld)
    dy = _rows(d.dy, lddy)
    x = _rows(d.x, ldx) if with_x else None
    y = _rows(y_relu, ldy) if y_relu is not None else None
    gamma, _beta, rm, rv = _stats(d)
    buf, dx = _guarded(M, lddx) if with_dx else (None, None)
    dg = torch.full((C,), float("nan"), device=DEV) if with_sums else None
    db = torch.full((C,), float("nan"), device=DEV) if with_sums else None
    sc = _scratch(lib, M, C) if with_sums else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())          # (the buffers above were filled on the current stream)
    L.check(lib.vidc_bn_eval_backward(L.ptr(dy), L.ptr(x), L.ptr(y), L.ptr(dx), M, C, lddy, ldx if with_x else 0, ldy if y is not None else 0,
                                      lddx if with_dx else 0, L.ptr(gamma), L.ptr(rm), L.ptr(rv), EPS, L.ptr(dg), L.ptr(db), L.ptr(sc),
                                      stream.cuda_stream if stream is not None else L.current_stream()), "bn eval backward")
    return dict(buf=buf, dx=dx, dg=dg, db=db, C=C, where="dx of (%d, %d, %d)" % (M, C, ld), keep=(dy, x, y, gamma, rm, rv, sc))


def _collect_backward(h):
    torch.cuda.synchronize()
    out = {}
    if h["dx"] is not None:
        _untouched(h["buf"], h["C"], h["where"])
        out["dx"] = h["dx"].cpu()[:, :h["C"]].contiguous()
    if h["dg"] is not None:
        out.update(dgamma=h["dg"].cpu(), dbeta=h["db"].cpu())
    return out


def _run_backward(*a, **k):
    return _collect_backward(_launch_backward(*a, **k))


@gpu
@pytest.mark.parametrize("M,C,ld", SHAPES, ids=_IDS)
def test_bn_eval_backward(M, C, ld):
    """With and without y_relu (an input: no gate is ambiguous, no element is left out): the full form (dx and the sums, two launches), the
    sums-only form (dx == NULL) and the no-sums form with x == NULL and no scratch (one launch).  dx, dgamma and dbeta against float64 under the
    bounds of the module docstring; the partial forms bit-equal to the full one; the same bits from two further calls enqueued on two streams before either result is read."""
    from vi_depth_completion_amd import _lib as L
    d = _data(M, C)
    side = torch.cuda.Stream()
    for y_in in (None, d.y_relu):
        ref = ref_backward(d.dy, d.x, y_in, d.gamma, d.rm, d.rv, EPS)
        where = "(%d, %d, %d) y_relu=%d" % (M, C, ld, y_in is not None)
        full = _run_backward(L, d, ld, y_in, True, True)
        _within("dx", full["dx"], ref["dx"], ref["dx_mag"], K_DX, where)
        _within("dgamma", full["dgamma"], ref["dgamma"], ref["dgamma_mag"], K_DGAMMA, where)
        _within("dbeta", full["dbeta"], ref["dbeta"], ref["dbeta_mag"], K_DBETA, where)
        assert float(full["dx"][:, d.gz].abs().max()) == 0.0, "gamma = 0: dx must be exact zeros"
        if y_in is not None:
            assert float(full["dx"][::3, 0].abs().max()) == 0.0 and float(full["dx"][1::3, 0].abs().max()) == 0.0, "y = +0 / -0 closes the gate"
        sums_only = _run_backward(L, d, ld, y_in, False, True)
        assert "dx" not in sums_only
        for k in ("dgamma", "dbeta"):
            assert _same_bits(sums_only[k], full[k]), "%s: %s of the sums-only form differs" % (where, k)
        dx_only = _run_backward(L, d, ld, y_in, True, False, with_x=False)
        assert _same_bits(dx_only["dx"], full["dx"]), "%s: dx of the no-sums form (x == NULL) differs from the full form's" % where
        pair = [_launch_backward(L, d, ld, y_in, True, True, stream=s) for s in (side, None)]      # neither waits for the other; read when both are done
        for again in [_collect_backward(h) for h in pair]:
            for k in ("dx", "dgamma", "dbeta"):
                assert _same_bits(again[k], full[k]), "%s: %s differs between two calls on two streams" % (where, k)
    _report("bn eval backward %s" % ((M, C, ld),))
