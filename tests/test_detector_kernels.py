"""The index kernels of the plane-mask detector (csrc/plane_mask.hip), one by one, at the smallest shapes that reach each of their branches.

tests/test_plane_mask.py reaches them through a PlaneMaskDetector at B = 1, 240x320, R = 50 on real-valued maps: W is a multiple of the
wave, ties never occur, and the level mapper / paste / select edge cases are whatever four frames produce.  Here every entry point is called
through the C ABI with its own buffers (pre-filled with NaN / 0xFF so that "not written" shows), B = 2 with different data per image, and
inputs built for the branches: both top-k paths at their smallest and largest n under masses of exact ties, empty levels, boxes on the
level mapper's boundaries, placeholders that survive NMS, truncation of negative paste corners, several rows inside one wave.

References are oracle/plane_mask_oracle.py (PM) and oracle/detector_oracle.py.  Where the oracle leaves an order unspecified (torch.topk /
torch.sort among equal values) a NumPy restatement applies the rule the kernel documents (lower index / lower level / lower slot first);
the unmarked CPU tests show every restatement equal to the oracle on untied inputs and establish the conditions the generated inputs
must meet (score separation, level boundaries, the size of the paste band).

Measured worst deviations on MI355X for the three float comparisons: profiles/EXPERIMENTS.md ("detector kernels one by one").
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detector_oracle as DO
from oracle import plane_mask_oracle as PM

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE = -2                                                   # VIDC_ERR_SHAPE (include/vidc.h)
LD = 32                                                          # row stride of the head / RPN / mask maps


def _L():
    from vi_depth_completion_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _i32(*shape, fill=-77):
    return torch.full(shape, fill, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ======================================================================================================================================
# 1. vidc_rpn_topk_decode / vidc_rpn_topk_decode_levels
# ======================================================================================================================================
TOPK_CASES = [(1, 1, 1000), (4, 5, 1000), (11, 31, 1000), (18, 19, 1000), (18, 19, 1024), (18, 19, 1), (18, 19, 1025), (43, 127, 1000),
              (43, 127, 2000)]
PATTERNS = "abcd"
GRID = np.arange(-8.0, 8.0 + 1e-9, 0.25).astype(np.float32)
FIVE = np.array([-3.0, -0.25, 0.5, 2.0, 6.25], np.float32)
SATURATED = np.array([20.0, 25.0, 30.0], np.float32)
IMAGE_SIZES = [(37, 53), (240, 320)]


@functools.lru_cache(maxsize=None)
def _rpn_map(h, w, pattern, stride=4):
    """(2, h, w, 32) fp32: channels 0..2 objectness logits in `pattern`, 3..14 box deltas, 15..31 junk nobody may read."""
    rng = np.random.RandomState(1000 * h + w + 17 * PATTERNS.index(pattern))
    m = rng.uniform(50, 60, (2, h, w, LD)).astype(np.float32)
    shape = (2, h, w, 3)
    if pattern == "a":
        lg = rng.choice(GRID, shape)
    elif pattern == "b":
        lg = np.broadcast_to(np.array([0.75, -2.5], np.float32).reshape(2, 1, 1, 1), shape).copy()
    elif pattern == "c":
        lg = rng.choice(FIVE, shape)
    else:
        lg = rng.choice(GRID, shape)
        sat = rng.uniform(size=shape) < 1.0 / 3
        lg[sat] = rng.choice(SATURATED, int(sat.sum()))
    d = rng.normal(0, 0.5, (2, h, w, 3, 4))
    kind = rng.uniform(size=(2, h, w, 3))
    big = kind < 0.12                                            # dw / dh above log(1000/16): the clamp
    d[big, 2:] = rng.uniform(4.2, 6.0, (int(big.sum()), 2))
    far = (kind > 0.8)                                           # offsets that push the box over an image edge, every edge in turn
    d[far, :2] = rng.choice([-1.0, 1.0], (int(far.sum()), 2)) * rng.uniform(3, 8, (int(far.sum()), 2))
    m[..., :3] = lg
    m[..., 3:15] = d.reshape(2, h, w, 12).astype(np.float32)
    return m


def _ref_sigmoid(logits):
    """torch's fp32 sigmoid, evaluated once per distinct logit.  torch.sigmoid itself is not a function of the value alone on the CPU: the
    vectorised body and the scalar tail of one tensor round differently (n = 1023, logit -7.5: element 1004 of 1023 comes out one ulp
    above the other fifteen), which would break ties that exist in the input.  Equal logits must be exact ties here."""
    vals, inverse = np.unique(np.asarray(logits, np.float32), return_inverse=True)
    return torch.from_numpy(vals).sigmoid().numpy()[inverse.reshape(np.shape(logits))]


def _topk_order(s, k):
    """The kernel's documented order: descending score, ascending index among equals."""
    return np.argsort(-s, kind="stable")[:k]


def _decode64(reg, anc, idx, hw):
    """PM.clip(PM.decode()) in float64 of the selected anchors, and the magnitude the box tolerance scales with."""
    d, a = torch.from_numpy(reg[idx].astype(np.float64)), anc[idx].double()
    want = PM.clip(PM.decode(d, a, (1.0, 1.0, 1.0, 1.0)), hw).numpy()
    d, a = d.numpy(), a.numpy()
    wd, ht = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
    pcx, pcy = d[:, 0] * wd + a[:, 0] + 0.5 * wd, d[:, 1] * ht + a[:, 1] + 0.5 * ht
    pw, ph = np.exp(np.minimum(d[:, 2], PM.BBOX_XFORM_CLIP)) * wd, np.exp(np.minimum(d[:, 3], PM.BBOX_XFORM_CLIP)) * ht
    return want, np.maximum.reduce([pw, ph, np.abs(pcx), np.abs(pcy)])


def _cell(stride, size):
    return np.ascontiguousarray(PM.cell_anchors(stride, size).numpy().astype(np.float32))


def _run_topk(m_dev, h, w, stride, cell, top_n, hw, k, pad=3):
    L = _L()
    boxes, scores = _nan(2, k + pad, 4), _nan(2, k + pad)
    L.check(L.lib().vidc_rpn_topk_decode(L.ptr(m_dev), 2, h, w, LD, 3, stride, cell.ctypes.data, top_n, hw[0], hw[1], L.ptr(boxes), L.ptr(scores),
                                         k + pad, L.current_stream()), "rpn_topk_decode")
    return boxes, scores


WORST = {}


def _note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))
    print("%s: %.3e (worst so far %.3e)" % (name, value, WORST[name]))


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("h,w,top_n", TOPK_CASES, ids=["%dx%d_top%d" % c for c in TOPK_CASES])
def test_rpn_topk_decode(h, w, top_n, pattern):
    """Exact order under ties (stable sort of the reference's fp32 sigmoid), scores to 1e-6, boxes against the float64 decode within
    1e-3 + 2e-6 max(pw, ph, |pcx|, |pcy|) (six fp32 roundings and expf at that magnitude), sentinel behind the k-th slot."""
    m = _rpn_map(h, w, pattern)
    n = 3 * h * w
    k = min(top_n, n)
    cell, anc = _cell(4, 32), PM.anchors((h, w), 4, 32)
    m_dev = _dev(m)
    for hw in IMAGE_SIZES:
        boxes, scores = _run_topk(m_dev, h, w, 4, cell, top_n, hw, k)
        boxes, scores = boxes.cpu().numpy(), scores.cpu().numpy()
        assert np.isnan(boxes[:, k:]).all() and np.isnan(scores[:, k:]).all(), "wrote behind the k-th slot"
        for b in range(2):
            s = _ref_sigmoid(m[b, :, :, :3].reshape(-1))
            order = _topk_order(s, k)
            err_s = np.abs(scores[b, :k].astype(np.float64) - s[order])
            print("image %d %s: score err %.2e" % (b, hw, err_s.max()))
            assert err_s.max() <= 1e-6
            want, mag = _decode64(m[b, :, :, 3:15].reshape(-1, 4), anc, order, hw)
            err = np.abs(boxes[b, :k].astype(np.float64) - want).max(1)
            tol = 1e-3 + 2e-6 * mag
            _note("rpn_topk_decode box err / tol", (err / tol).max())
            _note("rpn_topk_decode box err (px)", err.max())
            bad = np.flatnonzero(err > tol)
            assert bad.size == 0, "rank %d (anchor %d): %s vs %s" % (bad[0], order[bad[0]], boxes[b, bad[0]], want[bad[0]])


LEVELS = [((43, 127), 4, 32), ((18, 19), 8, 64), ((11, 31), 16, 128), ((4, 5), 32, 256), ((1, 1), 64, 512)]


@gpu
@pytest.mark.parametrize("pattern", ["a", "c"])
def test_rpn_topk_decode_levels_equals_single_level(pattern):
    """Five levels mixing the select path (n = 16383, 1026) and the sort path (1023, 60, 3) in one launch, offsets as _Buffers builds
    them: bit-equal to the single-level entry on every level."""
    L = _L()
    ks = [min(PM.PRE_NMS_TOP_N, 3 * h * w) for (h, w), _s, _z in LEVELS]
    off = np.concatenate(([0], np.cumsum(ks))).astype(np.int32)
    slots = int(off[-1])
    maps = [_dev(_rpn_map(h, w, pattern, s)) for (h, w), s, _z in LEVELS]
    cells = np.ascontiguousarray(np.stack([_cell(s, z) for _hw, s, z in LEVELS]))
    hw_arr = np.asarray([hw for hw, _s, _z in LEVELS], np.int32).copy()
    strides = np.asarray([s for _hw, s, _z in LEVELS], np.int32).copy()
    ptrs = (C.c_void_p * 5)(*[m.data_ptr() for m in maps])
    boxes, scores = _nan(2, slots, 4), _nan(2, slots)
    L.check(L.lib().vidc_rpn_topk_decode_levels(ptrs, hw_arr.ctypes.data, strides.ctypes.data, cells.ctypes.data, off.ctypes.data, 5, 2, LD, 3,
                                                PM.PRE_NMS_TOP_N, 240, 320, L.ptr(boxes), L.ptr(scores), slots, L.current_stream()), "levels")
    assert not torch.isnan(boxes).any() and not torch.isnan(scores).any()
    for l, ((h, w), s, _z) in enumerate(LEVELS):
        b1, s1 = _run_topk(maps[l], h, w, s, cells[l], PM.PRE_NMS_TOP_N, (240, 320), ks[l], pad=0)
        assert torch.equal(_bits(boxes[:, off[l]:off[l + 1]]), _bits(b1)), "level %d boxes" % l
        assert torch.equal(_bits(scores[:, off[l]:off[l + 1]]), _bits(s1)), "level %d scores" % l


@gpu
def test_rpn_topk_decode_refusals():
    L = _L()
    buf, cell = _nan(64), _cell(4, 32)
    st = L.current_stream()
    assert L.lib().vidc_rpn_topk_decode(L.ptr(buf), 2, 2, 2731, LD, 3, 4, cell.ctypes.data, 1000, 37, 53, L.ptr(buf), L.ptr(buf), 1000, st) == ERR_SHAPE
    assert L.lib().vidc_rpn_topk_decode(L.ptr(buf), 2, 4, 5, LD, 4, 4, cell.ctypes.data, 1000, 37, 53, L.ptr(buf), L.ptr(buf), 1000, st) == ERR_SHAPE
    ptrs, hw, one, off = (C.c_void_p * 1)(buf.data_ptr()), np.array([2, 2731], np.int32), np.array([4], np.int32), np.array([0, 1000], np.int32)
    for hw_l, A in ((hw, 3), (np.array([4, 5], np.int32), 4)):
        assert L.lib().vidc_rpn_topk_decode_levels(ptrs, hw_l.ctypes.data, one.ctypes.data, cell.ctypes.data, off.ctypes.data, 1, 2, LD, A, 1000, 37,
                                                   53, L.ptr(buf), L.ptr(buf), 1000, st) == ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


def test_topk_inputs_and_order_restatement():
    """The conditions behind test_rpn_topk_decode: neighbouring grid logits are >= 8e-5 apart in the fp32 sigmoid, {20, 25, 30} saturate to
    exactly 1.0f, every logit is inside [-30, 30], the cases reach the sizes the table names, and the stable order equals torch.topk
    wherever the k-th and the (k+1)-th value differ (always in values; in indices where a value is unique)."""
    sg = _ref_sigmoid(GRID)
    assert np.diff(sg).min() >= 8e-5 and (_ref_sigmoid(SATURATED) == np.float32(1.0)).all() and sg.max() < 1.0
    assert [3 * h * w for h, w, _k in TOPK_CASES] == [3, 60, 1023, 1026, 1026, 1026, 1026, 16383, 16383]
    for h, w, top_n in TOPK_CASES:
        for p in PATTERNS:
            m = _rpn_map(h, w, p)
            assert np.abs(m[..., :3]).max() <= 30 and np.isfinite(m).all()
            d = m[..., 3:15].reshape(-1, 4)
            assert (d[:, 2:] > PM.BBOX_XFORM_CLIP).any() or h * w < 20
            for b in range(2):
                s = _ref_sigmoid(m[b, :, :, :3].reshape(-1))
                assert np.abs(s.astype(np.float64) - torch.from_numpy(m[b, :, :, :3].reshape(-1).copy()).sigmoid().numpy()).max() <= 6e-8
                k = min(top_n, s.size)
                order = _topk_order(s, k)
                top, idx = torch.from_numpy(s).topk(k, sorted=True)
                assert np.array_equal(s[order], top.numpy())
                if k == s.size or np.sort(s)[::-1][k - 1] != np.sort(s)[::-1][k]:
                    assert np.array_equal(np.sort(order), np.sort(idx.numpy()))
                vals, counts = np.unique(s[order], return_counts=True)
                unique = np.isin(s[order], vals[counts == 1]) & (np.isin(s[order], s[np.setdiff1d(np.arange(s.size), order)]) == False)  # noqa: E712
                assert np.array_equal(order[unique], idx.numpy()[unique])
    # pattern (c) puts T inside a mass of ties, pattern (d) has more saturated scores than k
    s = _ref_sigmoid(_rpn_map(43, 127, "c")[0, :, :, :3].reshape(-1))
    assert np.sort(s)[::-1][999] == np.sort(s)[::-1][1000]
    assert (_ref_sigmoid(_rpn_map(43, 127, "d")[0, :, :, :3].reshape(-1)) == 1.0).sum() > 2000


# ======================================================================================================================================
# 2. vidc_rpn_select
# ======================================================================================================================================
def _select_ref(boxes, scores, keep, n_keep, off, per_level, total):
    """First min(n_keep, per_level) survivors of every level in level-major order, then a STABLE descending sort (ties: lower level, then
    earlier survivor, first); `total` slots, zeros behind the count."""
    B, nl = n_keep.shape
    props, ps, n = np.zeros((B, total, 4), np.float32), np.zeros((B, total), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        src = np.concatenate([off[l] + keep[b, off[l]:off[l] + min(n_keep[b, l], per_level)] for l in range(nl)]).astype(np.int64)
        order = np.argsort(-scores[b, src], kind="stable")[:total]
        n[b] = order.size
        props[b, :n[b]], ps[b, :n[b]] = boxes[b, src[order]], scores[b, src[order]]
    return props, ps, n


def _select_inputs(level_sizes, n_keep, seed, tied=True):
    """Per level: scores descending (the order NMS leaves), from a coarse grid when `tied` (equal scores inside and across levels), and
    a strictly increasing random `keep` list of n_keep survivors."""
    rng = np.random.RandomState(seed)
    n_keep = np.asarray(n_keep, np.int32)
    B, nl = n_keep.shape
    off = np.concatenate(([0], np.cumsum(level_sizes))).astype(np.int32)
    slots = int(off[-1])
    boxes = rng.uniform(0, 300, (B, slots, 4)).astype(np.float32)
    scores = np.zeros((B, slots), np.float32)
    keep = np.full((B, slots), 0, np.int32)
    for b in range(B):
        for l, sz in enumerate(level_sizes):
            sc = rng.randint(1, 33, sz) / 32.0 if tied else rng.permutation(B * slots)[:sz] / float(B * slots) * 0.9 + 0.05 + 1e-4 * (b * nl + l)
            scores[b, off[l]:off[l] + sz] = np.sort(sc.astype(np.float32))[::-1]
            keep[b, off[l]:off[l] + n_keep[b, l]] = np.sort(rng.permutation(sz)[:n_keep[b, l]])
    return boxes, scores, keep, n_keep, off


# (level sizes, n_keep [B][levels], per_level, total)
SELECT_CASES = {
    "five_levels_above_total": ([120, 90, 80, 60, 3], [[70, 50, 0, 13, 3], [50, 50, 50, 50, 3]], 50, 50),      # n_keep > per_level, a zero level
    "five_levels_below_total": ([120, 90, 80, 60, 3], [[7, 0, 5, 0, 1], [0, 0, 0, 0, 2]], 50, 50),
    "all_levels_empty": ([120, 90, 80, 60, 3], [[0, 0, 0, 0, 0], [3, 0, 0, 0, 0]], 50, 50),
    "one_level": ([200], [[64], [10]], 50, 50),
    "one_level_total_64": ([200], [[150], [0]], 100, 64),
    "five_levels_500_candidates": ([120, 110, 100, 100, 100], [[100, 100, 100, 100, 100], [100, 1, 100, 99, 100]], 100, 64),
}


def _run_select(inp, per_level, total):
    L = _L()
    boxes, scores, keep, n_keep, off = inp
    B, nl = n_keep.shape
    props, ps, n = _nan(B, total, 4), _nan(B, total), _i32(B)
    d_boxes, d_scores, d_keep, d_nk = _dev(boxes), _dev(scores), _dev(keep), _dev(n_keep)      # (named: they must outlive the launch)
    rc = L.lib().vidc_rpn_select(L.ptr(d_boxes), L.ptr(d_scores), L.ptr(d_keep), L.ptr(d_nk), B, nl, off.ctypes.data, per_level,
                                 total, L.ptr(props), L.ptr(ps), L.ptr(n), L.current_stream())
    return rc, props.cpu().numpy(), ps.cpu().numpy(), n.cpu().numpy()


@gpu
@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("case", sorted(SELECT_CASES))
def test_rpn_select(case, tied):
    sizes, n_keep, per_level, total = SELECT_CASES[case]
    inp = _select_inputs(sizes, n_keep, 5, tied)
    rc, props, ps, n = _run_select(inp, per_level, total)
    assert rc == 0, _L().lib().vidc_last_error()
    w_props, w_ps, w_n = _select_ref(*inp, per_level, total)
    assert np.array_equal(n, w_n), (n, w_n)
    assert np.array_equal(ps, w_ps), np.argwhere(ps != w_ps)[:4]                  # (NaN left anywhere fails both)
    assert np.array_equal(props, w_props), np.argwhere(props != w_props)[:4]
    if case == "all_levels_empty":
        assert n[0] == 0 and not props[0].any() and not ps[0].any()


@gpu
def test_rpn_select_refusal():
    inp = _select_inputs([100] * 6, [[1] * 6, [1] * 6], 0)
    rc, props, _ps, n = _run_select(inp, 100, 50)
    assert rc == ERR_SHAPE and np.isnan(props).all() and (n == -77).all()


def test_rpn_select_restatement_and_inputs():
    """Untied scores: the restatement equals the oracle's formulation (cat of the per-level survivors, torch.topk).  Tied inputs do hold
    equal scores across two levels, and the cases reach what their names say."""
    for case, (sizes, n_keep, per_level, total) in SELECT_CASES.items():
        boxes, scores, keep, nk, off = inp = _select_inputs(sizes, n_keep, 5, tied=False)
        props, ps, n = _select_ref(*inp, per_level, total)
        for b in range(nk.shape[0]):
            cat_b = torch.cat([torch.from_numpy(boxes[b, off[l]:off[l + 1]][keep[b, off[l]:off[l] + nk[b, l]][:per_level]]) for l in range(len(sizes))])
            cat_s = torch.cat([torch.from_numpy(scores[b, off[l]:off[l + 1]][keep[b, off[l]:off[l] + nk[b, l]][:per_level]]) for l in range(len(sizes))])
            assert cat_s.unique().numel() == cat_s.numel()
            top, order = torch.topk(cat_s, min(total, cat_s.numel()), sorted=True)
            assert n[b] == top.numel() and np.array_equal(ps[b, :n[b]], top.numpy()) and np.array_equal(props[b, :n[b]], cat_b[order].numpy())
            assert not props[b, n[b]:].any() and not ps[b, n[b]:].any()
        assert len(sizes) * per_level <= 512
    boxes, scores, keep, nk, off = _select_inputs(*SELECT_CASES["five_levels_above_total"][:2], 5, tied=True)
    lv0 = scores[0, off[0] + keep[0, off[0]:off[0] + 50]]
    lv1 = scores[0, off[1] + keep[0, off[1]:off[1] + 50]]
    assert np.intersect1d(lv0, lv1).size > 0


# ======================================================================================================================================
# 3. vidc_roi_align_fpn
# ======================================================================================================================================
FPN_HW = [(16, 24), (8, 12), (4, 6), (2, 3)]                     # P2..P5 of a 64x96 image
BOUNDARY_SIDES = [111, 112, 223, 224, 447, 448]
BOUNDARY_LEVELS = [2, 3, 3, 4, 4, 5]


def _square(x1, y1, side):
    return [x1, y1, x1 + side - 1, y1 + side - 1]


# R = 7, B = 2: the six boundary boxes and a tiny one on image 0; image 1: huge, zero-size, partly outside, entirely outside, and the
# boundary boxes 112 / 224 / 448 again (other features, other offsets)
FPN_BOXES = {
    7: [[_square(-20.0, -30.0, 111), _square(-10.0, -40.0, 112), _square(-100.0, -90.0, 223), _square(-64.0, -100.0, 224),
         _square(-200.0, -190.0, 447), _square(-180.0, -200.0, 448), [40.25, 20.5, 44.0, 23.75]],
        [[-900.0, -700.0, 1500.0, 1100.0], [30.5, 17.25, 29.5, 16.25], [70.3, 40.6, 130.9, 90.2], [300.0, 200.0, 340.0, 260.0],
         _square(3.0, -50.0, 112), _square(-120.0, -80.0, 224), _square(-170.0, -210.0, 448)]],
    1: [[_square(-10.0, -40.0, 112)], [[70.3, 40.6, 130.9, 90.2]]],
}


@functools.lru_cache(maxsize=None)
def _fpn_feats():
    g = torch.Generator().manual_seed(21)
    return tuple(torch.randn(2, 256, h, w, generator=g) * 2 + (3.0 if l == 1 else 0.0) for l, (h, w) in enumerate(FPN_HW))


def _pool_ref(feats, rois, resolution, sampling_ratio):
    """PM.pool with the sampling ratio as a parameter (PM.pool fixes 2)."""
    lv = PM.level_of(rois[:, 1:])
    out = torch.zeros(rois.shape[0], feats[0].shape[1], resolution, resolution)
    for l in range(4):
        idx = torch.nonzero(lv == l).squeeze(1)
        if idx.numel():
            out[idx] = torch.from_numpy(DO.roi_align_forward(feats[l].numpy(), rois[idx].numpy(), PM.POOLER_SCALES[l], resolution, resolution,
                                                              sampling_ratio))
    return out


def _rois(R):
    boxes = torch.tensor(FPN_BOXES[R], dtype=torch.float32)                          # (2, R, 4)
    return boxes, torch.cat((torch.arange(2.0).repeat_interleave(R)[:, None], boxes.view(-1, 4)), 1)


@functools.lru_cache(maxsize=None)
def _pool_want(R, pooled, sampling_ratio):
    """All 256 channels once; a test with fewer channels compares against the first C."""
    return _pool_ref(_fpn_feats(), _rois(R)[1], pooled, sampling_ratio)


@gpu
@pytest.mark.parametrize("sampling_ratio", [2, 0])
@pytest.mark.parametrize("pooled", [7, 14])
@pytest.mark.parametrize("R", [1, 7])
@pytest.mark.parametrize("Cn", [64, 100, 256])
def test_roi_align_fpn(Cn, R, pooled, sampling_ratio):
    L = _L()
    feats = [f[:, :Cn].permute(0, 2, 3, 1).contiguous().to(DEV) for f in _fpn_feats()]
    boxes, _ = _rois(R)
    want = _pool_want(R, pooled, sampling_ratio)[:, :Cn].permute(0, 2, 3, 1)
    ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])
    hw = np.asarray(FPN_HW, np.int32).copy()
    y, d_boxes = _nan(2 * R, pooled, pooled, Cn), boxes.to(DEV)
    L.check(L.lib().vidc_roi_align_fpn(ptrs, hw.ctypes.data, 4, Cn, L.ptr(d_boxes), 2, R, pooled, sampling_ratio, L.ptr(y), L.current_stream()),
            "roi_align_fpn")
    got = y.cpu()
    assert not torch.isnan(got).any()
    err, bar = float((got - want).abs().max()), 2e-5 * max(1.0, float(want.abs().max()))
    _note("roi_align_fpn err / bar", err / bar)
    per_box = (got - want).abs().flatten(1).max(1)[0]
    assert err <= bar, "worst box %d: %s" % (int(per_box.argmax()), per_box)


def test_roi_align_fpn_inputs():
    """PM.level_of on the boundary sides gives 2, 3, 3, 4, 4, 5 and keeps doing so when the area moves one ulp either way; the other boxes
    reach the clamps; the restatement with sampling_ratio = 2 is PM.pool; image 1 sees other features than image 0."""
    for side, lvl in zip(BOUNDARY_SIDES, BOUNDARY_LEVELS):
        area = np.float32(side) * np.float32(side)
        for a in (np.nextafter(area, np.float32(0)), area, np.nextafter(area, np.float32(np.inf))):
            got = torch.clamp(torch.floor(4 + torch.log2(torch.sqrt(torch.tensor(a)) / 224 + 1e-6)), min=2, max=5)
            assert int(got) == lvl, (side, a)
    boxes, rois = _rois(7)
    assert (PM.level_of(boxes[0]) + 2).tolist() == BOUNDARY_LEVELS + [2]
    assert (PM.level_of(boxes[1]) + 2).tolist() == [5, 2, 2, 2, 3, 4, 5]
    raw = 4 + torch.log2(torch.sqrt((boxes[..., 2] - boxes[..., 0] + 1) * (boxes[..., 3] - boxes[..., 1] + 1)) / 224 + 1e-6)
    assert raw[0, 6] < 2 and raw[1, 0] >= 6 and raw[1, 1] < 2                          # clamped below / above
    feats = _fpn_feats()
    assert torch.equal(_pool_want(7, 7, 2), PM.pool(list(feats), rois, 7))
    assert float(_pool_want(7, 7, 2)[10].abs().max()) == 0.0                            # the box entirely outside the map
    assert float(_pool_want(7, 7, 2)[9].abs().max()) > 0.0                             # the one partly outside
    assert all(not torch.equal(f[0], f[1]) for f in feats)


# ======================================================================================================================================
# 4. vidc_det_candidates -> vidc_nms_segmented -> vidc_det_select
# ======================================================================================================================================
DET_GRID = np.arange(-6.0, 6.0 + 1e-9, 0.5).astype(np.float32)   # plane logit minus background logit
DET_BASE = np.array([-1.0, 0.0, 1.0, 2.0], np.float32)           # the background logit that goes with each grid value: equal p <=> equal pair


def _det_inputs(R, n_props, hw, seed, background_image=None):
    """head (2*R, 32), props (2, R, 4).  Rows behind n_props hold a confident plane and far-away boxes: reading them would show."""
    rng = np.random.RandomState(seed)
    H, W = hw
    head = rng.uniform(50, 60, (2 * R, LD)).astype(np.float32)
    gi = rng.randint(0, DET_GRID.size, 2 * R)
    if background_image is not None:
        gi[background_image * R:(background_image + 1) * R] = rng.randint(0, 6, R)      # p <= sigmoid(-3.5): below SCORE_THRESH
    head[:, 0] = DET_BASE[gi % 4]
    head[:, 1] = DET_BASE[gi % 4] + DET_GRID[gi]
    head[:, 2:10] = rng.uniform(-2, 2, (2 * R, 8)).astype(np.float32)
    xy = np.stack([rng.uniform(0, W - 2, 2 * R), rng.uniform(0, H - 2, 2 * R)], 1)
    wh = np.stack([rng.uniform(1, W / 3, 2 * R), rng.uniform(1, H / 3, 2 * R)], 1)
    props = np.concatenate([xy, np.minimum(xy + wh, [W - 1, H - 1])], 1).astype(np.float32).reshape(2, R, 4)
    for b in range(2):
        head[b * R + n_props[b]:(b + 1) * R, :2] = [0.0, 9.0]
        props[b, n_props[b]:] = [5000.0, 5000.0, 9000.0, 9000.0]
    return head, props


def _cand_ref(head, props, n_props, R, hw):
    """Candidates in the kernel's documented order: plane probability > SCORE_THRESH, descending, lower proposal index first."""
    out = []
    for b in range(2):
        n = n_props[b]
        hd = torch.from_numpy(head[b * R:b * R + n])
        p1 = F.softmax(hd[:, :2], -1)[:, 1].numpy()
        ok = np.flatnonzero(p1 > np.float32(PM.SCORE_THRESH))
        src = ok[np.argsort(-p1[ok], kind="stable")]
        bx = PM.clip(PM.decode(hd[:, 2:10].double(), torch.from_numpy(props[b, :n]).double(), (10.0, 10.0, 5.0, 5.0)), hw)[:, 4:8].numpy()
        out.append((src, p1[src], bx[src]))
    return out


def _run_det_chain(head, props, n_props, R, hw):
    L = _L()
    lib, st = L.lib(), L.current_stream()
    hd, pr, npr = _dev(head), _dev(props), _dev(np.asarray(n_props, np.int32))
    cb, cs, csrc, nc = _nan(2, R, 4), _nan(2, R), _i32(2, R), _i32(2)
    keep, nkeep = _i32(2, R), _i32(2)
    db, ds, nd = _nan(2, R, 4), _nan(2, R), _i32(2)
    seg_off, seg_n = torch.arange(2, dtype=torch.int32, device=DEV) * R, torch.full((2,), R, dtype=torch.int32, device=DEV)
    scratch = torch.empty(lib.vidc_nms_segmented_scratch_bytes(2, R), dtype=torch.uint8, device=DEV)
    L.check(lib.vidc_det_candidates(L.ptr(hd), LD, L.ptr(pr), L.ptr(npr), 2, R, hw[0], hw[1], PM.SCORE_THRESH, L.ptr(cb), L.ptr(cs), L.ptr(csrc),
                                    L.ptr(nc), st), "det_candidates")
    L.check(lib.vidc_nms_segmented(L.ptr(cb), L.ptr(seg_off), L.ptr(seg_n), 2, R, PM.DET_NMS_THRESH, 1, 0, L.ptr(keep), L.ptr(nkeep), L.ptr(scratch), st),
            "nms_segmented")
    L.check(lib.vidc_det_select(L.ptr(cb), L.ptr(cs), L.ptr(csrc), L.ptr(nc), L.ptr(keep), L.ptr(nkeep), 2, R, L.ptr(db), L.ptr(ds), L.ptr(nd), st),
            "det_select")
    return [t.cpu().numpy() for t in (cb, cs, csrc, nc, nkeep, db, ds, nd)]


def _n_props_cases(R):
    return sorted({(0, R), (R, 0), (1, R // 2), (R // 2, 1), (R, R)})


DET_CASES = [(R, n, hw) for R, hw in ((1, (37, 53)), (50, (240, 320)), (64, (37, 53))) for n in _n_props_cases(R)]


@gpu
@pytest.mark.parametrize("R,n_props,hw", DET_CASES, ids=["R%d_n%d_%d" % (R, n[0], n[1]) for R, n, _hw in DET_CASES])
def test_det_chain(R, n_props, hw):
    """Candidates (count, order under tied scores, sources, placeholders), then the chain's detections against PM.detections per image."""
    head, props = _det_inputs(R, n_props, hw, 100 + R)
    cb, cs, csrc, nc, nkeep, db, ds, nd = _run_det_chain(head, props, n_props, R, hw)
    ref = _cand_ref(head, props, n_props, R, hw)
    for b in range(2):
        src, p1, bx = ref[b]
        n = src.size
        assert nc[b] == n and np.array_equal(csrc[b, :n], src) and (csrc[b, n:] == -1).all()
        assert np.abs(cs[b, :n] - p1).max(initial=0) <= 1e-5 and (cs[b, n:] == 0).all()
        assert np.abs(cb[b, :n] - bx).max(initial=0) <= 1e-3
        t = np.arange(n, R, dtype=np.float32)
        far = np.stack([np.float32(-1.0e6) - np.float32(10) * t, np.full(R - n, -1.0e6, np.float32)] * 2, 1)
        assert np.array_equal(cb[b, n:], far), "placeholders"
        assert nkeep[b] >= R - n                                                     # the placeholders overlap nothing: they survive NMS
        hd = torch.from_numpy(head[b * R:b * R + n_props[b]])
        wb, ws, _wl = PM.detections(hd[:, :2], hd[:, 2:10], torch.from_numpy(props[b, :n_props[b]]), hw)
        m = ws.numel()
        assert nd[b] == m, (nd[b], m)
        assert np.abs(db[b, :m] - wb.numpy()).max(initial=0) <= 1e-3 and np.abs(ds[b, :m] - ws.numpy()).max(initial=0) <= 1e-5
        assert not db[b, m:].any() and not ds[b, m:].any()                           # zeros, not NaN, behind the count
        assert db[b].min() >= 0                                                      # no placeholder among the detections


@gpu
@pytest.mark.parametrize("R", [50, 64])
def test_det_chain_all_background_image(R):
    """Image 0 has R proposals and none above SCORE_THRESH: R placeholders, all surviving NMS, none in the output; image 1 is ordinary."""
    hw = (240, 320)
    head, props = _det_inputs(R, (R, R), hw, 7, background_image=0)
    cb, cs, csrc, nc, nkeep, db, ds, nd = _run_det_chain(head, props, (R, R), R, hw)
    assert nc[0] == 0 and nkeep[0] == R and nd[0] == 0 and (csrc[0] == -1).all() and (cb[0] <= -1.0e6).all()
    assert not db[0].any() and not ds[0].any()
    assert nc[1] > 0 and nd[1] > 0 and db[1].min() >= 0
    wb, ws, _wl = PM.detections(torch.from_numpy(head[R:, :2]), torch.from_numpy(head[R:, 2:10]), torch.from_numpy(props[1]), hw)
    assert nd[1] == ws.numel() and np.abs(db[1, :nd[1]] - wb.numpy()).max() <= 1e-3


@gpu
def test_det_chain_refusal():
    L = _L()
    b, i = _nan(2 * 65 * LD), _i32(2 * 65)
    st = L.current_stream()
    assert L.lib().vidc_det_candidates(L.ptr(b), LD, L.ptr(b), L.ptr(i), 2, 65, 37, 53, 0.05, L.ptr(b), L.ptr(b), L.ptr(i), L.ptr(i), st) == ERR_SHAPE
    assert L.lib().vidc_det_select(L.ptr(b), L.ptr(b), L.ptr(i), L.ptr(i), L.ptr(i), L.ptr(i), 2, 65, L.ptr(b), L.ptr(b), L.ptr(i), st) == ERR_SHAPE


def test_det_inputs_and_restatement():
    """Plane probabilities are pairwise bit-equal or >= 1e-4 apart and >= 1e-3 from SCORE_THRESH; |deltas| <= 2; tied scores occur; and the
    candidate restatement, pushed through the oracle's NMS and put back in proposal order, is PM.detections."""
    pairs = torch.from_numpy(np.stack([DET_BASE[np.arange(DET_GRID.size) % 4], DET_BASE[np.arange(DET_GRID.size) % 4] + DET_GRID], 1))
    p = np.sort(F.softmax(pairs, -1)[:, 1].numpy().astype(np.float64))
    assert np.diff(p).min() >= 1e-4 and np.abs(p - PM.SCORE_THRESH).min() >= 1e-3
    for R, n_props, hw in DET_CASES:
        head, props = _det_inputs(R, n_props, hw, 100 + R)
        assert np.abs(head[:, 2:10]).max() <= 2
        for b, (src, p1, bx) in enumerate(_cand_ref(head, props, n_props, R, hw)):
            hd = torch.from_numpy(head[b * R:b * R + n_props[b]])
            allp = F.softmax(hd[:, :2], -1)[:, 1].numpy().astype(np.float64)
            gaps = np.abs(allp[:, None] - allp[None, :])
            assert ((gaps == 0) | (gaps >= 1e-4)).all()
            if R == 64 and n_props[b] == 64:
                assert np.unique(p1).size < p1.size                                  # tied candidates
            keep = PM.nms(torch.from_numpy(bx).float(), torch.from_numpy(p1), PM.DET_NMS_THRESH).numpy()
            sel = np.sort(src[keep])
            wb, ws, _wl = PM.detections(hd[:, :2], hd[:, 2:10], torch.from_numpy(props[b, :n_props[b]]), hw)
            assert np.array_equal(ws.numpy(), allp[sel].astype(np.float32)) or np.allclose(ws.numpy(), allp[sel], atol=1e-7)
            assert ws.numel() == sel.size


# ======================================================================================================================================
# 5. vidc_mask_paste
# ======================================================================================================================================
# in units of (W - 1, H - 1): negative expanded corners that truncate to 0 (not floor to -1), one pixel, the whole image, over the
# bottom-right, thin and fractional, ordinary
PASTE_UNIT_BOXES = [(0.004, 0.011, 0.36, 0.358), (0.583, 0.572, 0.583, 0.572), (0.0, 0.0, 1.0, 1.0), (0.77, 0.69, 1.16, 1.27),
                    (0.196, 0.155, 0.879, 0.169), (0.106, 0.229, 0.591, 0.847)]
PASTE_SIZES = [(37, 53), (9, 11)]
PASTE_R = 7
BAND = 1e-5


@functools.lru_cache(maxsize=None)
def _paste_inputs(M, hw):
    """Mask logits (2*R, M, M) = 3 N(0, 1) and boxes (2, R, 4); image 1 has the boxes in reverse order; slot 6 is never a detection."""
    H, W = hw
    g = torch.Generator().manual_seed(3)
    logits = (3 * torch.randn(2 * PASTE_R, M, M, generator=g)).numpy()
    bx = np.array([[x0 * (W - 1), y0 * (H - 1), x1 * (W - 1), y1 * (H - 1)] for x0, y0, x1, y1 in PASTE_UNIT_BOXES], np.float32)
    boxes = np.full((2, PASTE_R, 4), 3.0, np.float32)
    boxes[0, :6], boxes[1, :6] = bx, bx[::-1]
    return logits, boxes


def _paste_ref64(logits, boxes, hw, M):
    """float64 restatement of PM.paste_masks for K slots: masks (K, H, W) uint8, the band |p - 0.5| <= BAND, the in-box pixels."""
    H, W = hw
    MP = M + 2
    K = boxes.shape[0]
    out, band, inbox = np.zeros((K, H, W), np.uint8), np.zeros((K, H, W), bool), np.zeros((K, H, W), bool)
    for k in range(K):
        padded = np.zeros((MP, MP))
        padded[1:-1, 1:-1] = 1.0 / (1.0 + np.exp(-logits[k].astype(np.float64)))
        b = boxes[k].astype(np.float64)
        scale = MP / M
        wh, hh, xc, yc = (b[2] - b[0]) * .5 * scale, (b[3] - b[1]) * .5 * scale, (b[2] + b[0]) * .5, (b[3] + b[1]) * .5
        bx0, by0, bx1, by1 = (int(math.trunc(v)) for v in (xc - wh, yc - hh, xc + wh, yc + hh))
        bw, bh = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
        for y in range(max(by0, 0), min(by1 + 1, H)):
            sy = max(MP / bh * (y - by0 + 0.5) - 0.5, 0.0)
            y0 = int(sy); y1 = y0 + (1 if y0 < MP - 1 else 0); ly = sy - y0
            for x in range(max(bx0, 0), min(bx1 + 1, W)):
                sx = max(MP / bw * (x - bx0 + 0.5) - 0.5, 0.0)
                x0 = int(sx); x1 = x0 + (1 if x0 < MP - 1 else 0); lx = sx - x0
                v = (1 - ly) * ((1 - lx) * padded[y0, x0] + lx * padded[y0, x1]) + ly * ((1 - lx) * padded[y1, x0] + lx * padded[y1, x1])
                out[k, y, x], band[k, y, x], inbox[k, y, x] = v > 0.5, abs(v - 0.5) <= BAND, True
    return out, band, inbox


@functools.lru_cache(maxsize=None)
def _paste_want(M, hw):
    logits, boxes = _paste_inputs(M, hw)
    return _paste_ref64(logits, boxes.reshape(-1, 4), hw, M)


def _paste_layout(logits, M, cls, seed=0):
    """(K, M, M) -> the conv engine's [K][M/2][M/2 * 4][ld] with mask pixel (py, px) at [py/2][(px/2)*4 + (py&1)*2 + (px&1)], channel cls."""
    K = logits.shape[0]
    out = np.random.RandomState(seed).normal(0, 3, (K, M // 2, M // 2 * 4, LD)).astype(np.float32)
    py, px = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    out[:, py >> 1, (px >> 1) * 4 + (py & 1) * 2 + (px & 1), cls] = logits
    return out


@gpu
@pytest.mark.parametrize("n_det", [(6, 0), (0, 6), (6, 6)])
@pytest.mark.parametrize("cls", [0, 1, 31])
@pytest.mark.parametrize("hw", PASTE_SIZES, ids=["37x53", "9x11"])
@pytest.mark.parametrize("M", [28, 4])
def test_mask_paste(M, hw, cls, n_det):
    L = _L()
    H, W = hw
    logits, boxes = _paste_inputs(M, hw)
    want, band, _inbox = _paste_want(M, hw)
    want, band = want.reshape(2, PASTE_R, H, W), band.reshape(2, PASTE_R, H, W)
    out = torch.full((2, PASTE_R, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    d_logits, d_boxes, d_n = _dev(_paste_layout(logits, M, cls)), _dev(boxes), _dev(np.asarray(n_det, np.int32))
    L.check(L.lib().vidc_mask_paste(L.ptr(d_logits), LD, cls, M, L.ptr(d_boxes), L.ptr(d_n), 2, PASTE_R, H, W, 0.5, L.ptr(out), L.current_stream()),
            "mask_paste")
    got = out.cpu().numpy()
    assert got.max() <= 1, "a pixel was not written"
    for b in range(2):
        assert not got[b, n_det[b]:].any(), "slots behind n_det must be zero"
        diff = (got[b, :n_det[b]] != want[b, :n_det[b]]) & ~band[b, :n_det[b]]
        assert not diff.any(), "image %d: %d pixels differ outside the band, first at %s" % (b, diff.sum(), np.argwhere(diff)[:1])


def test_mask_paste_restatement_and_band():
    """The float64 restatement reproduces PM.paste_masks on these inputs, at most 0.1 % of the in-box pixels lie within 1e-5 of the
    threshold (sample coordinate <= 30 at 6e-8 relative error, slope <= 1 per unit, four fp32 products), and the boxes reach their
    branches: a negative corner that truncates towards 0 where floor would not (to 0 at M = 28), a 1x1 box, corners below -1 and beyond W, H."""
    for M in (28, 4):
        for hw in PASTE_SIZES:
            H, W = hw
            logits, boxes = _paste_inputs(M, hw)
            want, band, inbox = _paste_want(M, hw)
            prob = torch.from_numpy(logits).sigmoid()[:, None]
            assert np.array_equal(want, PM.paste_masks(prob, torch.from_numpy(boxes.reshape(-1, 4)), hw).numpy()), (M, hw)
            print("M = %d, %dx%d: %d of %d in-box pixels in the band" % (M, H, W, band.sum(), inbox.sum()))
            assert band.sum() <= 1e-3 * inbox.sum()
            assert want[:6].reshape(6, -1).any(1).sum() >= 4 and inbox[1].sum() == 1
            b = boxes[0].astype(np.float64)
            s = (M + 2) / M
            x0 = (b[:, 2] + b[:, 0]) * .5 - (b[:, 2] - b[:, 0]) * .5 * s
            x1 = (b[:, 2] + b[:, 0]) * .5 + (b[:, 2] - b[:, 0]) * .5 * s
            assert x0[0] < 0 and (M != 28 or x0[0] > -1) and x0[0] != np.floor(x0[0]) and x0[2] < 0 and (W < 50 or x0[2] <= -1) and x1[3] > W and b[1, 0] == b[1, 2] and b[1, 1] == b[1, 3]


# ======================================================================================================================================
# 6. vidc_instance_map
# ======================================================================================================================================
CCL_SHAPES = [(9, 11), (20, 40), (16, 64), (13, 65), (37, 53), (30, 100)]
CONFIDENCE = float(np.float32(0.9))


def _instance_ref(masks, scores, hw, confidence):
    """PM.instance_map with the kernel's documented tie rule for equal scores: lower slot first (a stable sort; torch.sort's order among
    equal values is unspecified).  Equal sizes keep the score order in both (sorted() is stable)."""
    from scipy import ndimage
    keep = np.flatnonzero(scores > np.float32(confidence))
    keep = keep[np.argsort(-scores[keep], kind="stable")]
    planes = []
    for k in keep:
        binary = (masks[k] != 0).astype(np.uint8)
        lab, nb = ndimage.label(binary)
        sz = ndimage.sum(binary, lab, range(nb + 1))
        m = ((sz == max(sz)) & (sz > 0))[lab]
        planes.append((int(m.sum()), m))
    inst, index = np.zeros(hw, np.uint8), 1
    for size, m in sorted(planes, key=lambda t: t[0], reverse=True):
        if size >= 0.05 * hw[0] * hw[1]:
            inst[m] = index
            index += 1
    return inst


def _threshold_px(hw):
    return int(math.ceil(0.05 * hw[0] * hw[1]))


def _raster(hw, n):
    m = np.zeros(hw[0] * hw[1], np.uint8)
    m[:n] = 1
    return m.reshape(hw)


def _blocks(hw):
    """(q, c): a q x c block is smaller than the 5 % threshold t, two of them (minus one pixel) reach it."""
    t = _threshold_px(hw)
    s = (t + 2) // 2
    c = max(1, min(hw[1] // 2 - 1, s))
    return -(-s // c), c


def _designed(hw, rng):
    """The twelve designed masks of one (H, W)."""
    H, W = hw
    t = _threshold_px(hw)
    q, c = _blocks(hw)
    yy, xx = np.mgrid[:H, :W]
    edge = np.zeros(hw, np.uint8)                                # last column of rows 1, 3, ... plus first column of the rows after them
    edge[1:H - 1:2, W - 1] = 1
    edge[2:H:2, 0] = 1
    edge[0, :max(2, t // (H // 2) + 1)] = 0
    twin = np.zeros(hw, np.uint8)                                # two components of the same, maximal size: kept together, sized by their sum
    twin[1:1 + q, :c] = 7
    twin[2 + q:2 + 2 * q, W - c:] = 255
    twin[H - 1, W // 2] = 1
    wrap = np.zeros(hw, np.uint8)                                # q*c and q*c - 1 pixels that touch only through the row wrap-around
    wrap[2:2 + q, W - c:] = 1
    wrap[2 + q:2 + 2 * q, :c] = 1
    wrap[2 + 2 * q - 1, c - 1] = 0
    left, right = np.zeros(hw, np.uint8), np.zeros(hw, np.uint8)  # equal sizes, partial overlap: the painting order shows
    n_cols = (3 * W) // 5
    left[:, :n_cols], right[:, W - n_cols:] = 1, 1
    return [(rng.uniform(size=hw) < 0.3).astype(np.uint8), (rng.uniform(size=hw) < 0.5).astype(np.uint8), (rng.uniform(size=hw) < 0.7).astype(np.uint8),
            np.ones(hw, np.uint8), ((yy + xx) % 2 == 0).astype(np.uint8), edge, twin, _raster(hw, t), _raster(hw, t - 1), wrap, left, right]


@functools.lru_cache(maxsize=None)
def _ccl_case(hw, R, tied):
    """masks (2, R, H, W), scores (2, R), n_det (2,).  Image 0: the designed masks (then noise); image 1: a slot whose score equals the
    confidence exactly, noise, and behind n_det garbage masks with high scores."""
    rng = np.random.RandomState(31 * hw[0] + hw[1] + R)
    masks = (rng.uniform(size=(2, R) + hw) < rng.uniform(0.2, 0.8, (2, R, 1, 1))).astype(np.uint8)
    scores = (0.86 + 0.139 * (rng.permutation(2 * R) + 0.5) / (2 * R)).astype(np.float32).reshape(2, R)      # distinct, some below 0.9
    designed = _designed(hw, rng)
    if R == 1:
        masks[0, 0], scores[0, 0] = designed[5], 0.95
        n_det = (1, 0)
        scores[1, 0] = 0.99
    else:
        masks[0, :12] = designed
        scores[0, :12] = np.float32(0.999) - np.float32(0.004) * rng.permutation(12).astype(np.float32)
        scores[1, 0] = CONFIDENCE
        n_det = (R, 5 if R == 12 else 40)
        scores[1, n_det[1]:] = 0.9999
        if tied:
            scores[0, 10] = scores[0, 11] = 0.97                 # `left` and `right`: equal score, equal size
            scores[0, 0] = scores[0, 2] = scores[0, 3]
            scores[1, 1] = scores[1, 2] = scores[1, 3] = 0.95
    return masks, scores, n_det


def _ccl_want(hw, R, tied):
    masks, scores, n_det = _ccl_case(hw, R, tied)
    return np.stack([_instance_ref(masks[b, :n_det[b]], scores[b, :n_det[b]], hw, CONFIDENCE) for b in range(2)])


@gpu
@pytest.mark.parametrize("R", [1, 12, 64])
@pytest.mark.parametrize("hw", CCL_SHAPES, ids=["%dx%d" % s for s in CCL_SHAPES])
def test_instance_map(hw, R):
    L = _L()
    H, W = hw
    for tied in ((False,) if R == 1 else (False, True)):
        masks, scores, n_det = _ccl_case(hw, R, tied)
        want = _ccl_want(hw, R, tied)
        if not tied:
            for b in range(2):
                assert np.array_equal(want[b], PM.instance_map(torch.from_numpy(masks[b, :n_det[b]]), torch.from_numpy(scores[b, :n_det[b]]), hw, CONFIDENCE))
        inst = torch.full((2, H, W), 0xFF, dtype=torch.uint8, device=DEV)
        scratch = torch.full((L.lib().vidc_instance_map_scratch_bytes(2, R, H, W),), 0xFF, dtype=torch.uint8, device=DEV)
        d_masks, d_scores, d_n = _dev(masks), _dev(scores), _dev(np.asarray(n_det, np.int32))
        L.check(L.lib().vidc_instance_map(L.ptr(d_masks), L.ptr(d_scores), L.ptr(d_n), 2, R, H, W, CONFIDENCE, 0.05, L.ptr(inst), L.ptr(scratch),
                                          L.current_stream()), "instance_map")
        got = inst.cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b], want[b]), "tied=%s image %d: %d pixels differ\n%s\n%s" % (tied, b, (got[b] != want[b]).sum(), got[b], want[b])


def test_instance_map_restatement_and_inputs():
    """The restatement is PM.instance_map on every untied case; a raster of exactly ceil(5 %) pixels is kept and one pixel less is
    dropped (40 and 39 px at 20x40); the wrap-around slot is dropped although its two blocks together would pass; the twin slot passes only
    by the sum of its two components; the edge mask's last-column and first-column pixels are separate components; equal scores exist
    in the tied cases only."""
    from scipy import ndimage
    one = np.array([0.95], np.float32)
    assert _threshold_px((20, 40)) == 40 and _threshold_px((30, 100)) == 150
    for hw in CCL_SHAPES:
        t = _threshold_px(hw)
        d = _designed(hw, np.random.RandomState(0))
        q, c = _blocks(hw)
        assert _instance_ref(d[7][None], one, hw, CONFIDENCE).sum() == t and d[7].sum() == t
        assert _instance_ref(d[8][None], one, hw, CONFIDENCE).sum() == 0 and d[8].sum() == t - 1
        assert q * c < t <= 2 * q * c - 1 and d[9].sum() == 2 * q * c - 1 and ndimage.label(d[9])[1] == 2
        assert d[9].reshape(-1)[(2 + q) * hw[1] - 1] and d[9].reshape(-1)[(2 + q) * hw[1]]           # neighbours in memory, not in the image
        assert _instance_ref(d[9][None], one, hw, CONFIDENCE).sum() == 0
        assert (_instance_ref(d[6][None], one, hw, CONFIDENCE) == 1).sum() == 2 * q * c and ndimage.label(d[6])[1] == 3
        assert ndimage.label(d[5])[1] == d[5].sum() and d[5].sum() >= 4
        flat = d[5].reshape(-1)
        assert (flat[:-1] & flat[1:]).sum() >= 2                                                     # last column next to a first column
        assert _instance_ref(d[5][None], one, hw, CONFIDENCE).sum() in (0, d[5].sum())
        assert d[10].sum() == d[11].sum() and (d[10] & d[11]).any() and (d[10] != d[11]).any()
        for R in (1, 12, 64):
            masks, scores, n_det = _ccl_case(hw, R, False)
            want = _ccl_want(hw, R, False)
            for b in range(2):
                live = scores[b, :n_det[b]][scores[b, :n_det[b]] > CONFIDENCE]
                assert np.unique(live).size == live.size
                assert np.array_equal(want[b], PM.instance_map(torch.from_numpy(masks[b, :n_det[b]]), torch.from_numpy(scores[b, :n_det[b]]), hw, CONFIDENCE))
            if R > 1:
                assert scores[1, 0] == np.float32(CONFIDENCE) and n_det[1] < R and (scores[1, n_det[1]:] > 0.99).all()
                ts = _ccl_case(hw, R, True)[1]
                assert ts[0, 10] == ts[0, 11] and ts[1, 1] == ts[1, 2]
    # the score-tie rule shows: swapping the painting order of `left` and `right` changes the expected map
    masks, scores, n_det = _ccl_case((20, 40), 12, True)
    a = _instance_ref(masks[0, 10:12], scores[0, 10:12], (20, 40), CONFIDENCE)
    b = _instance_ref(masks[0, [11, 10]], scores[0, [11, 10]], (20, 40), CONFIDENCE)
    assert not np.array_equal(a, b)


# ======================================================================================================================================
# 7. vidc_det_stem_im2col / vidc_upsample_nearest2x
# ======================================================================================================================================
IM2COL_SIZES = [(5, 7), (33, 31), (64, 96), (37, 53)]


def _special_pixels():
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.array([0.0, 1.0], np.float32)])


@functools.lru_cache(maxsize=None)
def _stem_image(hw):
    """(2, 3, H, W) in [0, 1]: every k/255 with its two fp32 neighbours, 0, 1 and uniform noise, shuffled (a small image holds a sample)."""
    rng = np.random.RandomState(hw[0] * 100 + hw[1])
    n = 2 * 3 * hw[0] * hw[1]
    sp = _special_pixels()
    vals = np.concatenate([sp, rng.uniform(0, 1, max(n - sp.size, sp.size // 4)).astype(np.float32)])
    return torch.from_numpy(rng.permutation(vals)[:n].reshape(2, 3, *hw).copy())


def _im2col_ref(img):
    x, _hw = PM.preprocess(img)
    B, _c, Hp, Wp = x.shape
    cols = F.unfold(x, 7, padding=3, stride=2).view(B, 3, 49, Hp // 2, Wp // 2)       # channel-major (c, kh*7 + kw)
    return cols.permute(0, 3, 4, 2, 1).reshape(B, Hp // 2, Wp // 2, 147), (Hp, Wp)    # k = (kh*7 + kw)*3 + c


@gpu
@pytest.mark.parametrize("hw", IM2COL_SIZES, ids=["%dx%d" % s for s in IM2COL_SIZES])
def test_det_stem_im2col(hw):
    """|diff| <= 1e-4 (values <= 255; (u8 / 255) * 255 - mean may be contracted into one FMA: four ulps of 255); a different uint8
    decision would show as >= 1.  The 13 pad columns are exactly 0."""
    L = _L()
    img = _stem_image(hw)
    want, (Hp, Wp) = _im2col_ref(img)
    cols, d_img = _nan(2, Hp // 2, Wp // 2, 160), img.to(DEV)
    mb, mg, mr = PM.PIXEL_MEAN
    L.check(L.lib().vidc_det_stem_im2col(L.ptr(d_img), L.ptr(cols), 2, hw[0], hw[1], Hp, Wp, mb, mg, mr, L.current_stream()), "det_stem_im2col")
    got = cols.cpu()
    assert torch.equal(got[..., 147:], torch.zeros(2, Hp // 2, Wp // 2, 13))
    err = float((got[..., :147] - want).abs().max())
    _note("det_stem_im2col err", err)
    assert err <= 1e-4


def test_det_stem_im2col_inputs():
    sp = _special_pixels()
    assert sp.size == 770 and sp.min() > -1e-30 and sp.max() < 1.0000002
    for hw in IM2COL_SIZES:
        img = _stem_image(hw)
        assert float(img.min()) > -1e-30 and float(img.max()) < 1.0000002
        if 6 * hw[0] * hw[1] >= 2 * sp.size:
            assert np.isin(sp, img.numpy()).all()
        want, (Hp, Wp) = _im2col_ref(img)
        assert Hp % 32 == 0 and Wp % 32 == 0 and want.shape == (2, Hp // 2, Wp // 2, 147)
    # the rearrangement: tap (kh, kw) of channel c (BGR) of output pixel (oy, ox) reads preprocess()[c, 2 oy - 3 + kh, 2 ox - 3 + kw]
    img = _stem_image((33, 31))
    want, _ = _im2col_ref(img)
    x, _ = PM.preprocess(img)
    assert want[1, 5, 4, (2 * 7 + 6) * 3 + 1] == x[1, 1, 2 * 5 - 3 + 2, 2 * 4 - 3 + 6]
    u8 = (255.0 * img).to(torch.uint8)
    assert int(u8.min()) == 0 and int(u8.max()) == 255


@gpu
@pytest.mark.parametrize("Cn,ldx,ldy", [(4, 4, 4), (4, 8, 12), (256, 256, 256), (256, 260, 264)])
def test_upsample_nearest2x(Cn, ldx, ldy):
    L = _L()
    h, w = 5, 7
    g = torch.Generator().manual_seed(Cn + ldx)
    x = torch.randn(2, h, w, ldx, generator=g)
    y, d_x = _nan(2, 2 * h, 2 * w, ldy), x.to(DEV)
    L.check(L.lib().vidc_upsample_nearest2x(L.ptr(d_x), L.ptr(y), 2, h, w, Cn, ldx, ldy, L.current_stream()), "upsample_nearest2x")
    got = y.cpu()
    want = x[..., :Cn].repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(_bits(got[..., :Cn]), _bits(want))
    assert torch.isnan(got[..., Cn:]).all()                                          # the gap of every row is untouched


@gpu
def test_upsample_nearest2x_refusal():
    L = _L()
    x, y = _nan(2 * 5 * 7 * 8), _nan(2 * 10 * 14 * 8)
    assert L.lib().vidc_upsample_nearest2x(L.ptr(x), L.ptr(y), 2, 5, 7, 6, 8, 8, L.current_stream()) == ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
