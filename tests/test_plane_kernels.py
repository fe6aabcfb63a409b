"""The plane block's kernels (csrc/plane.hip), entry by entry through the C ABI, at the smallest shapes that reach each of their branches.

tests/test_plane.py and tests/test_hip_parity.py reach them through PlaneBlock at 240x320 on real-valued noise and accept a few "borderline"
pixels.  Here every entry is called with buffers the test owns (pre-filled with NaN / 0xFF / -77, each with a guard region behind it, the
scratch exactly vidc_plane_scratch_bytes long), B = 2 with different data per image, slots from both images in no particular order with the
plane ids 1, 7 and 255, HW = 63 / 256 / 1961 / 4160 (less than a wave, one chunk, odd with a partial last chunk and the scalar path of the
sparse list, a multiple of 4 just above 4096) and 240x320 once.

Two kinds of input.  EXACT scenes: classes of constant normals (0, 0, -+1) and homo = (0, 0, 2^k), dot products on a 2^-12 grid, so that
n_bar, the mean angle, n.P, every sum in any order, the offset and the projected depth are exact and everything is compared for equality.
NOISY scenes: random normals / depths whose decisions carry margins (checked in float64 by the unmarked tests below), so that any correct
fp32 evaluation takes every decision like the float64 restatement: masks, counts, ranks, flags and pixel sets are compared for equality, and
only n_bar, the mean angle, the offset and the written depths within a bound = 4 x the deviation of the fp32 oracle from float64 on these
very inputs (the kernel sums in another order).  Measured on MI355X: profiles/EXPERIMENTS.md ("plane kernels one by one").

The references are float64 NumPy restatements of oracle/vidc_oracle.py; the unmarked tests hold them against the oracle's functions.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import vidc_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_NULL, ERR_SHAPE = -1, -2                                       # include/vidc.h
MAX_HYP, REC, CH, GUARD = 300, 16, 256, 64
F32 = np.float32
THR_DIST, THR_DOT, THR_FRAC = float(F32(0.1)), float(F32(1e-3)), F32(0.05)
SMALL = [(7, 9), (16, 16), (37, 53), (65, 64)]
IDS = ["%dx%d" % s for s in SMALL]
SLOT_ORDER = [(1, 7), (0, 255), (1, 1), (0, 1), (1, 255), (0, 7)]  # both images, not ascending
N_HYP = {(1, 7): 64, (0, 255): 300, (1, 1): 1, (0, 1): 2, (1, 255): 299, (0, 7): 65}
N_PTS = {(0, 7): 301, (0, 255): 300, (0, 1): 2, (1, 7): 0, (1, 1): 1, (1, 255): 299}


def _L():
    from vi_depth_completion_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Out:
    """A device output pre-filled with `fill`, GUARD untouchable elements behind it."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[:n].view(*shape)
        self.guard = self.whole[n:].clone()

    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        assert torch.equal(self.whole[self.t.numel():].view(torch.uint8), self.guard.view(torch.uint8)), "the guard region was written"
        return self.t.cpu().numpy()


# ======================================================================================================================================
# scenes
# ======================================================================================================================================
def _ids(HW, b):
    """Plane-id map of image b.  HW >= 1024, image 0: class 7 holds 256 / 255 / 1 / 0 pixels of the chunks 0..3, class 1 one pixel of
    chunk 1; behind them (and in image 1) the classes interleave.  HW < 1024: interleaved, class 1 of image 0 is ONE pixel."""
    p = np.arange(HW)
    if HW < 1024:
        ids = np.array([[7, 255, 1, 0, 7, 7, 255, 0], [255, 0, 1, 1, 7, 0, 255, 255]], np.uint8)[b][p % 8]
        if b == 0:
            ids[ids == 1] = 0
            ids[HW - 1] = 1
        return ids
    if b == 1:
        return np.array([1, 7, 255, 0], np.uint8)[p % 4]
    ids = np.array([7, 255, 1, 7, 255, 0], np.uint8)[p % 6]
    ids[:511], ids[511], ids[512], ids[513:768], ids[768:1024] = 7, 1, 7, 255, 0
    return ids


def _slots_for(ids, hyp_rows):
    """slots int32 [n][4] and hyp_pix from {(b, cls): rows into the class's ascending pixel list}, in SLOT_ORDER."""
    slots, hyp, off = [], [], 0
    for b, cls in SLOT_ORDER:
        if (b, cls) not in hyp_rows:
            continue
        pix = np.flatnonzero(ids[b] == cls)
        hyp.append(pix[hyp_rows[(b, cls)]])
        slots.append((b, cls, off, len(hyp[-1])))
        off += len(hyp[-1])
    return np.asarray(slots, np.int32).reshape(-1, 4), np.concatenate(hyp).astype(np.int32)


def _designed_rows(ids, rng, background_image=None):
    rows = {}
    for b, cls in SLOT_ORDER:
        n = int((ids[b] == cls).sum())
        if n and b != background_image:
            rows[(b, cls)] = rng.permutation(n)[:min(N_HYP[(b, cls)], n)]
    return rows


@functools.lru_cache(maxsize=None)
def _exact_scene(H, W, tie=None):
    """Constant normals (0, 0, -1) on four of five class pixels and (0, 0, +1) on the fifth, homo = (0, 0, z) with z in {1/2, 1, 2}, sparse
    points t / z with t on a 2^-12 grid: cluster A = 1 + k/4096 (three of four points) and cluster B = 1.5 + k/4096, k < 301 distinct per
    point.  Junk depths on the background and on the class pixels outside the inlier mask.  At (7, 9) image 1 is background only; image 1
    of (16, 16) has no sparse depth.  `tie` = "a" / "b": the slot (0, 255) gets two clusters of EQUAL size whose first point in row-major
    order belongs to cluster A / B (and whose last one to the other)."""
    HW = H * W
    rng = np.random.RandomState(H * 1000 + W)
    bg = 1 if HW == 63 else None
    ids = np.stack([_ids(HW, 0), _ids(HW, 1) if bg is None else np.zeros(HW, np.uint8)])
    normals = np.zeros((2, 3, HW), F32)
    normals[:, 0], normals[:, 2] = 0.6, 0.8                        # background: never read for a decision
    for b in range(2):
        for cls in (1, 7, 255):
            pix = np.flatnonzero(ids[b] == cls)
            normals[b, :, pix] = 0
            normals[b, 2, pix] = np.where(np.arange(pix.size) % 5 == 4, 1.0, -1.0)
    slots, hyp = _slots_for(ids, _designed_rows(ids, rng, bg))
    homo = np.zeros((2, HW, 3), F32)
    homo[:, :, 2] = np.array([0.5, 1.0, 2.0], F32)[np.arange(HW) % 3]
    sc = {"H": H, "W": W, "ids": ids, "normals": normals, "slots": slots, "hyp": hyp, "homo": homo, "depth": np.zeros((2, HW), F32), "exact": True}
    stage1 = _ref_chain(sc)                                        # the masks decide where the points go
    depth = np.zeros((2, HW), F32)
    depth[ids == 0] = np.where(np.arange(2 * HW).reshape(2, HW) % 2 == 0, 5.0, 0.0)[ids == 0]
    for k, (b, cls, _o, _n) in enumerate(slots):
        mask = stage1["mask"][k].astype(bool)
        depth[b, (ids[b] == cls) & ~mask] = 3.25
        inl = np.flatnonzero(mask)
        n = min(N_PTS[(b, cls)], inl.size)
        at = inl[np.sort(rng.permutation(inl.size)[:n])]
        t = np.where(np.arange(n) % 4 == 3, 1.5, 1.0) + rng.permutation(301)[:n] / 4096.0
        if tie and (b, cls) == (0, 255):
            n -= n % 2
            at, first = at[:n], np.arange(n) % 2 == (0 if tie == "a" else 1)
            t = np.where(first, 1.0, 1.5) + rng.permutation(301)[:n] / 4096.0
        depth[b, at] = t / homo[b, at, 2]
    if HW == 256:
        depth[1] = 0
    sc["depth"] = depth.astype(F32)
    return sc


BASE = {1: (0.1, -0.2, -0.97), 7: (-0.3, 0.1, -0.95), 255: (0.2, 0.3, -0.93)}
PLANE_D = {1: 1.5, 7: 2.5, 255: 3.5}
COS_LO, COS_HI = np.cos(np.radians(20.005)), np.cos(np.radians(19.995))
COS_SURE, COS_NEVER = F32(0.93969262078590838) + F32(1e-4), F32(0.93969262078590838) - F32(1e-4)      # csrc/plane.hip


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _noisy_scene(H, W, drawn=0, density=(0.7, 0.1)):
    """Normals = a direction per class + N(0, 0.12) per component (a spread of several degrees), 15 % of them anywhere; a pinhole homo; sparse
    depths on `density` of the pixels of image 0 / 1: the class's plane * (1 + N(0, 0.03)), a fifth of them 1.4 x as far.  Normals are redrawn
    until no (hypothesis, class pixel) angle lies within 5e-3 degrees of 20.  `drawn` = seed: the hypotheses are the ones PlaneBlock draws from
    RandomState(seed) (slots ascending, min(300, size) rows each), else the designed ones (SLOT_ORDER, N_HYP)."""
    HW = H * W
    rng = np.random.RandomState(H * 1000 + W + 7)
    ids = np.stack([_ids(HW, 0), _ids(HW, 1)])
    if drawn:
        from vi_depth_completion_amd import plane
        slots, hyp, _ = plane.draw_normal_hypotheses([m.reshape(H, W) for m in ids], np.random.RandomState(drawn))
    else:
        slots, hyp = _slots_for(ids, _designed_rows(ids, rng))
    normals = _unit(rng.normal(size=(2, HW, 3)))

    def draw(cls, n):
        v = _unit(np.asarray(BASE[cls]) + 0.12 * rng.normal(size=(n, 3)))
        far = rng.uniform(size=n) < 0.15
        v[far] = _unit(rng.normal(size=(int(far.sum()), 3)))
        return v.astype(F32).astype(np.float64)

    for b in range(2):
        for cls in (1, 7, 255):
            pix = np.flatnonzero(ids[b] == cls)
            normals[b, pix] = draw(cls, pix.size)
    normals = normals.astype(F32).astype(np.float64)
    for b, cls, off, n in slots:
        hp, pix = hyp[off:off + n], np.flatnonzero(ids[b] == cls)
        for _ in range(200):                                       # the hypotheses among themselves first, then every other class pixel
            c = normals[b, hp] @ normals[b, hp].T
            bad = np.unique(hp[((c > COS_LO) & (c < COS_HI)).any(0)])
            if bad.size == 0:
                break
            normals[b, bad] = draw(cls, bad.size)
        todo = pix
        for _ in range(200):
            c = normals[b, hp] @ normals[b, todo].T
            todo = todo[((c > COS_LO) & (c < COS_HI)).any(0)]
            assert not np.isin(todo, hp).any()
            if todo.size == 0:
                break
            normals[b, todo] = draw(cls, todo.size)
    y, x = np.mgrid[0:H, 0:W]
    f = 0.8 * W
    homo = np.stack([(x - W / 2) / f, (y - H / 2) / f, np.ones((H, W))], -1).reshape(1, HW, 3).repeat(2, 0).astype(F32)
    depth = np.zeros((2, HW))
    for b in range(2):
        true = np.full(HW, 2.0)
        for cls in (1, 7, 255):
            m = ids[b] == cls
            true[m] = -PLANE_D[cls] / (homo[b, m].astype(np.float64) @ _unit(np.asarray(BASE[cls])))
        meas = true * (1 + 0.03 * rng.normal(size=HW)) * np.where(rng.uniform(size=HW) < 0.2, 1.4, 1.0)
        depth[b] = np.where(rng.uniform(size=HW) < density[b], meas, 0.0)
    depth = depth.astype(F32)
    for b, cls, off, n in slots:                                   # no two points of a plane at a distance within 5e-6 of 0.1: nudge one
        mask, n_bar = _ref_normal(normals[b].T, ids[b] == cls, hyp[off:off + n])[2:4]
        pts = np.flatnonzero(mask & (depth[b] > 0))
        for _ in range(100):
            dots = (homo[b, pts].astype(np.float64) * depth[b, pts].astype(np.float64)[:, None]) @ n_bar
            bad = np.unique(np.nonzero(np.triu(np.abs(np.abs(dots[:, None] - dots[None, :]) - THR_DIST) < 5e-6))[1])
            if bad.size == 0:
                break
            depth[b, pts[bad]] *= F32(1) + F32(1e-4) * rng.uniform(1, 2, bad.size).astype(F32)
    return {"H": H, "W": W, "ids": ids, "normals": np.ascontiguousarray(normals.transpose(0, 2, 1)).astype(F32), "slots": slots, "hyp": hyp,
            "homo": homo, "depth": depth, "exact": False}


# ======================================================================================================================================
# float64 restatement of the whole chain (oracle/vidc_oracle.py: mean_normal_ransac, plane_offset_ransac, generate_depth_from_plane,
# extract_plane_depth), slot by slot, with the kernels' documented rules: first maximal row wins, fp32 thresholds.
# ======================================================================================================================================
def _div(s, n, exact):
    """s / n: in fp32 where s is exact (the kernel's one rounding), in float64 otherwise."""
    return float(F32(s) / F32(n)) if exact else s / n


def _ref_normal(N, cm, hp):
    """N (3, HW) float64, cm the class's pixels, hp the hypothesis pixels -> counts, winner row, mask, n_bar, mean angle, smallest distance of
    an angle from 20 degrees."""
    ang = np.degrees(np.arccos(np.clip(N[:, hp].T @ N[:, cm], -1.0, 1.0)))
    close = ang < 20.0
    counts = close.sum(1)
    win = int(np.argmax(counts))
    mask = np.zeros(N.shape[1], bool)
    mask[np.flatnonzero(cm)[close[win]]] = True
    n_bar, mean_angle = np.zeros(3), 0.0
    if mask.any():
        m = N[:, mask].mean(1)
        n_bar = m / max(np.linalg.norm(m), 1e-12)
        mean_angle = float(np.abs(np.degrees(np.arccos(np.clip(n_bar @ N[:, mask], -1, 1)))).mean())
    return counts, win, mask, n_bar, mean_angle, ang


def _ref_offset(dots, idx, exact):
    """plane_offset_ransac on the dots n.P (row-major order) with the hypothesis ranks idx -> offset, n inliers, margin to 0.1."""
    if dots.size == 0:
        return 0.0, 0, np.inf
    if dots.size == 1:
        return -float(dots[0]), 1, np.inf
    dist = np.abs(-dots[idx][:, None] + dots[None, :])
    inl = dist < THR_DIST
    bi = int(np.argmax(inl.sum(1)))
    n = int(inl[bi].sum())
    return -_div(dots[inl[bi]].sum(), n, exact), n, float(np.abs(dist - THR_DIST).min())


def _ref_project(n_bar, off, mean_depth, mask, homo, out):
    """generate_depth_from_plane -> valid, n projected, margin of |n.homo| to 1e-3; writes `out` when valid."""
    dots = (homo[:, 0] * n_bar[0] + homo[:, 1] * n_bar[1]) + homo[:, 2] * n_bar[2]
    ok = mask & (np.abs(dots) > THR_DOT)
    vals = -off / dots[ok]
    n = int(ok.sum())
    valid = True
    if n:
        if F32((vals > mean_depth * 10.0).sum()) / F32(n) > THR_FRAC or (vals > 10.0).any() or (vals < 0).any():
            valid = False
    if valid:
        out[ok] = vals
    return valid, n, float(np.abs(np.abs(dots[mask]) - THR_DOT).min(initial=np.inf))


def _ref_chain(sc, dense=None, depth=None):
    """dense: {slot: ranks [300]} for the slots with more than 300 points (None: such a slot is flagged like a first pass)."""
    ids, slots, exact = sc["ids"], sc["slots"], sc["exact"]
    depth = (sc["depth"] if depth is None else depth).astype(np.float64)
    HW = ids.shape[1]
    n = slots.shape[0]
    out = {"counts": np.zeros((n, MAX_HYP), np.int32), "mask": np.zeros((n, HW), np.uint8), "rec": np.zeros((n, REC)), "dots": [],
           "pd": depth.copy(), "m_angle": np.inf, "m_dist": np.inf, "m_dot": np.inf, "written": np.zeros((2, HW), bool)}
    for k, (b, cls, off, nh) in enumerate(slots):
        N, homo, rec = sc["normals"][b].astype(np.float64), sc["homo"][b].astype(np.float64), out["rec"][k]
        counts, win, mask, n_bar, mean_angle, ang = _ref_normal(N, ids[b] == cls, sc["hyp"][off:off + nh])
        out["counts"][k, :nh], out["mask"][k] = counts, mask
        out["m_angle"] = min(out["m_angle"], np.abs(ang - 20.0).min())
        rec[0:3], rec[4], rec[5], rec[6], rec[12] = n_bar, mask.sum(), mean_angle, float(mask.any() and not mean_angle > 20.0), win
        out["dots"].append(np.zeros(0))
        if not rec[6]:
            continue
        vd = mask & (depth[b] > 0)
        dots = (homo[vd] * depth[b, vd][:, None]) @ n_bar
        out["dots"][k] = dots
        rec[7] = dots.size
        if dots.size > MAX_HYP and (dense is None or k not in dense):
            rec[6], rec[10] = 0.0, -1.0
            continue
        rec[8] = _div(depth[b, vd].sum(), dots.size, exact) if dots.size else 0.0
        rec[3], rec[9], m = _ref_offset(dots, dense[k] if dots.size > MAX_HYP else np.arange(dots.size), exact)
        out["m_dist"] = min(out["m_dist"], m)
        if rec[9] == 0:
            continue
        before = out["pd"][b].copy()
        valid, rec[11], m = _ref_project(n_bar, rec[3], rec[8], mask, homo, out["pd"][b])
        out["written"][b] |= before.view(np.int64) != out["pd"][b].view(np.int64)
        rec[10] = float(valid)
        out["m_dot"] = min(out["m_dot"], m)
    keep = depth > 0
    out["pd"][keep] = depth[keep]
    out["written"] &= ~keep
    nc = -(-HW // CH)
    gt = np.zeros((2, nc * CH), bool)
    gt[:, :HW] = out["pd"] > 0
    out["info"] = np.concatenate([gt.reshape(2, nc, CH).sum(2).reshape(-1), [(out["rec"][:, 10] < 0).sum()]]).astype(np.int32)
    return out


class _Replay:
    """A generator whose permutation() hands out prepared arrays in turn."""

    def __init__(self, arrays):
        self.arrays = list(arrays)

    def permutation(self, _a):
        return np.asarray(self.arrays.pop(0))


def _oracle32(sc, dense=None):
    """The oracle's own fp32 functions chained the way O.extract_plane_depth chains them, with this scene's hypothesis rows."""
    ids, slots, HW = sc["ids"], sc["slots"], sc["ids"].shape[1]
    depth, res = torch.from_numpy(sc["depth"]), []
    pd = depth.clone()
    for k, (b, cls, off, nh) in enumerate(slots):
        m = torch.from_numpy(ids[b] == cls)
        pix = np.flatnonzero(ids[b] == cls)
        nimg, homo = torch.from_numpy(sc["normals"][b].T.copy()), torch.from_numpy(sc["homo"][b]).view(1, HW, 3)
        rows = np.searchsorted(pix, sc["hyp"][off:off + nh])
        n_bar, ang, best, _ = O.mean_normal_ransac(nimg[m], num_hyp=int(nh), rng=_Replay([rows]))
        m2 = m.clone()
        m2[m] = best
        r = {"mask": m2.numpy(), "n_bar": n_bar.numpy(), "mean_angle": float(ang.abs().mean()), "offset": 0.0, "n_off": 0, "valid": None}
        res.append(r)
        if ang.abs().mean() > O.MEAN_NORMAL_ANGLE_DIFF_THR:
            continue
        vd = m2 & (depth[b] > 0)
        pc = homo[0][vd] * depth[b][vd][:, None]
        if pc.shape[0] > MAX_HYP and (dense is None or k not in dense):
            continue
        o, r["n_off"] = O.plane_offset_ransac(n_bar, pc.T, rng=_Replay([dense[k]] if pc.shape[0] > MAX_HYP else []))
        if r["n_off"] == 0:
            continue
        r["offset"] = float(o)
        eq = torch.cat([n_bar, torch.as_tensor(o, dtype=torch.float32).view(1)])
        img = pd[b].view(1, HW)
        r["valid"] = bool(O.generate_depth_from_plane(eq, m2.view(1, HW), homo, img, torch.mean(depth[b][vd])))
    keep = depth > 0
    pd[keep] = depth[keep]
    return res, pd.numpy()


def _dense_for(sc, seed=3):
    """The second pass's draws: 300 ranks for every slot the first pass flags (slot -> ranks), and the n_pts they were drawn for."""
    first = _ref_chain(sc)
    rng = np.random.RandomState(seed)
    flagged = np.flatnonzero(first["rec"][:, 10] < 0)
    dense = {int(k): rng.permutation(int(first["rec"][k, 7]))[:MAX_HYP].astype(np.int32) for k in flagged}
    if dense:
        dense["n_pts"] = {int(k): int(first["rec"][k, 7]) for k in flagged}
    return dense, first


@functools.lru_cache(maxsize=None)
def _bounds():
    """4 x the largest deviation of the fp32 oracle from the float64 restatement over the noisy scenes of SMALL (with their second pass), for
    n_bar, the mean angle (degrees), the offset and the written depths."""
    dev = {"n_bar": 0.0, "mean_angle": 0.0, "offset": 0.0, "depth": 0.0}
    for H, W in SMALL:
        sc = _noisy_scene(H, W)
        dense, _ = _dense_for(sc)
        want = _ref_chain(sc, dense)
        res, pd = _oracle32(sc, dense)
        for k, r in enumerate(res):
            dev["n_bar"] = max(dev["n_bar"], np.abs(r["n_bar"] - want["rec"][k, 0:3]).max())
            dev["mean_angle"] = max(dev["mean_angle"], abs(r["mean_angle"] - want["rec"][k, 5]))
            dev["offset"] = max(dev["offset"], abs(r["offset"] - want["rec"][k, 3]))
        dev["depth"] = max(dev["depth"], np.abs(pd - want["pd"]).max())
    return {q: 4 * v for q, v in dev.items()}, dev


# ======================================================================================================================================
# running the entries
# ======================================================================================================================================
def _run(sc, dense=None, depth=None, shift=0, block=False, dense_n=None, n_slots=None):
    """The five entries in order (block: vidc_plane_block) on buffers of exactly the documented sizes.  dense: None = vidc_plane_offset;
    {slot: ranks} = vidc_plane_offset_dense with dense_n[slot] = `dense_n` or the reference's n_pts, 0 elsewhere.  shift: the depth
    pointer starts `shift` floats into its allocation.  Returns numpy arrays (the guards checked)."""
    L = _L()
    lib, st = L.lib(), L.current_stream()
    ids, slots = sc["ids"], sc["slots"]
    B, HW = ids.shape
    n = slots.shape[0] if n_slots is None else n_slots
    room = torch.zeros(B * HW + 8, dtype=torch.float32, device=DEV)
    d = room[shift:shift + B * HW]
    d.copy_(_dev(sc["depth"] if depth is None else depth).view(-1))
    nrm, idd, sl, hp, homo = _dev(sc["normals"]), _dev(ids), _dev(slots), _dev(sc["hyp"]), _dev(sc["homo"])
    m = max(n, 1)
    mask, counts, rec = _Out((m, HW), torch.uint8, 0xFF), _Out((m, MAX_HYP), torch.int32, -77), _Out((m, REC), torch.float32, float("nan"))
    scratch = _Out((lib.vidc_plane_scratch_bytes(m, B, HW),), torch.uint8, 0xFF)
    pd, info = _Out((B, HW), torch.float32, float("nan")), _Out((lib.vidc_plane_info_count(B, HW),), torch.int32, -77)
    dh = dn = dots = None
    if dense is not None:
        h_dh, h_dn = np.zeros((m, MAX_HYP), np.int32), np.zeros(m, np.int32)
        for k, n_pts in (dense.get("n_pts", {}) if dense_n is None else dense_n).items():
            h_dh[k], h_dn[k] = dense[k], n_pts
        dh, dn, dots = _dev(h_dh), _dev(h_dn), _Out((m, HW), torch.float32, float("nan"))
    P = L.ptr
    if block:
        L.check(lib.vidc_plane_block(P(nrm), P(idd), P(sl), n, P(hp), B, HW, P(homo), P(d), mask.ptr(), counts.ptr(), scratch.ptr(), rec.ptr() if n else None,
                                     P(dh), P(dn), dots.ptr() if dots else None, pd.ptr(), info.ptr(), st), "plane_block")
    else:
        pd.t.copy_(d.view(B, HW))
        if n:
            L.check(lib.vidc_plane_ransac_normal(P(nrm), P(idd), P(sl), n, P(hp), HW, mask.ptr(), counts.ptr(), scratch.ptr(), st), "ransac_normal")
            if dense is None:
                L.check(lib.vidc_plane_offset(P(homo), P(d), P(sl), n, B, mask.ptr(), counts.ptr(), HW, scratch.ptr(), rec.ptr(), st), "offset")
            else:
                L.check(lib.vidc_plane_offset_dense(P(homo), P(d), P(sl), n, B, mask.ptr(), counts.ptr(), HW, scratch.ptr(), rec.ptr(), P(dh), P(dn),
                                                    dots.ptr(), st), "offset_dense")
            L.check(lib.vidc_plane_project_depth(P(homo), P(sl), n, mask.ptr(), HW, scratch.ptr(), rec.ptr(), pd.ptr(), st), "project_depth")
        L.check(lib.vidc_plane_finalize(P(d), pd.ptr(), B, HW, rec.ptr() if n else None, n, info.ptr(), st), "finalize")
    torch.cuda.synchronize()
    scratch.np()
    got = {"mask": mask.np(), "counts": counts.np(), "rec": rec.np(), "pd": pd.np(), "info": info.np(), "dots": dots.np() if dots else None}
    assert torch.equal(room[:shift], torch.zeros_like(room[:shift])) and not room[shift + B * HW:].any()
    return got


WORST = {}


def _note(name, value, bound):
    WORST[name] = max(WORST.get(name, 0.0), float(value))
    print("%s: %.3e, bound %.3e (worst so far %.3e)" % (name, value, bound, WORST[name]))


def _compare(sc, got, want, depth=None):
    """Decisions for equality on every scene; the four float quantities for equality on an exact scene, within _bounds() on a noisy one."""
    slots, exact = sc["slots"], sc["exact"]
    depth = sc["depth"] if depth is None else depth
    n, HW = slots.shape[0], sc["ids"].shape[1]
    rec = got["rec"]
    assert got["mask"].max() <= 1, "a mask byte is neither 0 nor 1"
    assert np.array_equal(got["counts"], want["counts"]), np.argwhere(got["counts"] != want["counts"])[:4]      # unused columns: zero
    assert np.array_equal(got["mask"], want["mask"]), np.argwhere(got["mask"] != want["mask"])[:4]
    assert not np.isnan(rec).any()
    for f in (4, 6, 7, 9, 10, 11, 12):
        assert np.array_equal(rec[:, f], want["rec"][:, f].astype(F32)), (f, rec[:, f], want["rec"][:, f])
    assert not rec[:, 13:].any()
    for k in range(n):
        assert rec[k, 4] == got["counts"][k, int(rec[k, 12])] == got["mask"][k].sum()
    if got["dots"] is not None:
        for k in range(n):
            w = want["dots"][k]
            if exact:
                assert np.array_equal(got["dots"][k, :w.size], w.astype(F32)), "slot %d: the on-plane points are not in row-major order" % k
            else:
                assert np.abs(got["dots"][k, :w.size] - w).max(initial=0) <= 2e-6 * 8, k
            assert np.isnan(got["dots"][k, w.size:]).all()
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    wrote = got["pd"].view(np.int32) != np.ascontiguousarray(depth, F32).view(np.int32)
    assert np.array_equal(wrote, want["written"]), "the set of written pixels differs"
    if exact:
        for f in (0, 1, 2, 3, 5, 8):
            assert np.array_equal(rec[:, f], want["rec"][:, f].astype(F32)), (f, rec[:, f], want["rec"][:, f])
        assert (rec[rec[:, 4] > 0, 5] == 0).all()
        assert np.array_equal(got["pd"], want["pd"].astype(F32))
    else:
        bound, _ = _bounds()
        tag = "%dx%d " % (sc["H"], sc["W"])
        for name, dev in (("n_bar", np.abs(rec[:, 0:3] - want["rec"][:, 0:3]).max()), ("mean_angle", np.abs(rec[:, 5] - want["rec"][:, 5]).max()),
                          ("offset", np.abs(rec[:, 3] - want["rec"][:, 3]).max()), ("depth", np.abs(got["pd"] - want["pd"]).max())):
            _note(tag + name, dev, bound[name])
        assert np.abs(rec[:, 8] - want["rec"][:, 8]).max() <= 1e-5
        assert np.abs(rec[:, 0:3] - want["rec"][:, 0:3]).max() <= bound["n_bar"]
        assert np.abs(rec[:, 5] - want["rec"][:, 5]).max() <= bound["mean_angle"]
        assert np.abs(rec[:, 3] - want["rec"][:, 3]).max() <= bound["offset"]
        assert np.abs(got["pd"] - want["pd"]).max() <= bound["depth"]


# ======================================================================================================================================
# 1. vidc_plane_ransac_normal (records read back through vidc_plane_offset on an all-zero depth)
# ======================================================================================================================================
@gpu
@pytest.mark.parametrize("kind", ["exact", "noisy"])
@pytest.mark.parametrize("H,W", SMALL, ids=IDS)
def test_ransac_normal(H, W, kind):
    """Counts of n_hyp = 1, 2, 64, 65, 299, 300 rows (as far as the class has pixels), unused columns zero, mask bytes 0 / 1, winner row,
    n_bar, mean angle, accepted; rec[4] == counts[slot, rec[12]] == mask[slot].sum().  Classes of one pixel, smaller than a chunk, with
    256 / 255 / 1 / 0 pixels in a chunk."""
    sc = _exact_scene(H, W) if kind == "exact" else _noisy_scene(H, W)
    zero = np.zeros_like(sc["depth"])
    got, want = _run(sc, depth=zero), _ref_chain(sc, depth=zero)
    _compare(sc, got, want, depth=zero)
    assert not got["rec"][:, 3].any() and not got["rec"][:, 7:12].any()
    assert not got["pd"].any()


def _special_scene():
    """(16, 16), B = 2.  Class 7 of both images: clusters 90 degrees apart -- 38 pixels (1, 0, 0) with xa, xb at 15 degrees on either side
    of them (30 degrees from each other), 30 pixels (0, 1, 0), 20 pixels (0, 0, 1); a hypothesis on xa and one on xb count 39 each, every
    other row fewer.  Class 1 of image 0: the hypothesis (0, 0, -1) and pixels at 19.99 / 20.01 / 19 / 21 / 5 / 60 degrees from it on eight
    azimuths, and two whose dot with it equals fl(cos 20 + 1e-4f) and fl(cos 20 - 1e-4f), the ends of the kernel's acosf band.  Class 255 of image 0: 30 identical normals (0.6, 0.8, 0.01), self-dot 1.0001.  Class 255 of image 1: all-zero normals.
    Class 1 of image 1: one pixel."""
    HW = 256
    rng = np.random.RandomState(5)
    ids, normals = np.zeros((2, HW), np.uint8), np.zeros((2, 3, HW), F32)
    normals[:, 1] = 1.0
    cl = {}
    for b in range(2):
        pix = rng.permutation(HW)
        cl[b] = {"core": pix[:38], "xa": pix[38], "xb": pix[39], "y": pix[40:70], "z": pix[70:90], "rest": pix[90:]}
        ids[b, pix[:90]] = 7
        normals[b][:, pix[:90]] = 0
        normals[b][0, pix[:38]], normals[b][1, pix[40:70]], normals[b][2, pix[70:90]] = 1, 1, 1
        c, s = np.cos(np.radians(15.0)), np.sin(np.radians(15.0))
        normals[b][:, pix[38]], normals[b][:, pix[39]] = (c, s, 0), (c, -s, 0)
    band = cl[0]["rest"][:51]
    ids[0, band] = 1
    th = np.radians(np.repeat([19.99, 20.01, 19.0, 21.0, 5.0, 60.0], 8))
    az = np.tile(np.arange(8) * np.pi / 4 + 0.1, 6)
    normals[0][:, band[0]] = (0, 0, -1)
    normals[0][:, band[1:49]] = np.stack([np.sin(th) * np.cos(az), np.sin(th) * np.sin(az), -np.cos(th)])
    for p, c in ((band[49], COS_SURE), (band[50], COS_NEVER)):     # dots that EQUAL the ends of the kernel's band (19.98 / 20.02 degrees)
        normals[0][:, p] = (np.sqrt(1 - float(c) ** 2), 0, -c)
    same = cl[0]["rest"][51:81]
    ids[0, same] = 255
    normals[0][:, same] = np.array([[0.6], [0.8], [0.01]], F32)
    zero = cl[1]["rest"][:25]
    ids[1, zero] = 255
    normals[1][:, zero] = 0
    ids[1, cl[1]["rest"][30]] = 1
    slots, hyp, expect = [], [], []
    for i, (lo, hi) in enumerate([(0, 1), (3, 70), (63, 64), (64, 128), (5, 299)]):
        for swap in (False, True):
            b = i % 2
            rows = np.concatenate([cl[b]["y"], cl[b]["z"]])[rng.randint(0, 50, MAX_HYP)]
            rows[lo], rows[hi] = (cl[b]["xb"], cl[b]["xa"]) if swap else (cl[b]["xa"], cl[b]["xb"])
            slots.append((b, 7, len(hyp) * MAX_HYP, MAX_HYP))
            hyp.append(rows)
            expect.append((lo, hi, rows[lo], rows[hi]))
    hyp = list(np.concatenate(hyp))
    for b, cls, rows in ((0, 1, [band[0]]), (0, 255, list(same[[3, 0, 7]])), (1, 255, list(zero[[2, 1]])), (1, 1, [cl[1]["rest"][30]])):
        slots.append((b, cls, len(hyp), len(rows)))
        hyp += rows
    homo = np.zeros((2, HW, 3), F32)
    homo[:, :, 2] = 1
    return {"H": 16, "W": 16, "ids": ids, "normals": normals, "slots": np.asarray(slots, np.int32), "hyp": np.asarray(hyp, np.int32), "homo": homo,
            "depth": np.zeros((2, HW), F32), "exact": False}, expect, band


@gpu
def test_ransac_normal_ties_band_clamp_and_zero_normals():
    """Ties go to the lower row -- pairs (0, 1), (3, 70), (63, 64), (64, 128), (5, 299): across neighbouring lanes, across lanes of different
    scan rounds, across the wave's ends, inside one lane's scan -- and swapping the two rows' pixels keeps the index and swaps the mask.
    Pixels at 20 +- 0.01 degrees (inside the acosf band of the kernel, 170 x fp32's noise) are decided as in float64, and so are the two whose
    dot equals an end of that band: the count and the mask must treat them alike (the count kernel once left the upper end to neither of
    its two paths, one pixel short of the mask).  Normals whose self-dot
    exceeds 1 are clamped: mean angle exactly 0, not NaN.  An all-zero-normal class: every count 0, winner row 0, empty mask, rec[4] =
    rec[6] = 0 -- the oracle "accepts" such a plane (its mean over no inliers is NaN, and NaN > 20 is false) and then finds no points on
    its empty mask, so neither writes a depth."""
    sc, expect, band = _special_scene()
    got, want = _run(sc), _ref_chain(sc)
    rec, ids = got["rec"], sc["ids"]
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["mask"], want["mask"])
    for k, (lo, hi, p_lo, p_hi) in enumerate(expect):
        c = got["counts"][k]
        assert c[lo] == c[hi] == 39 == c.max() and (c == 39).sum() == 2
        assert rec[k, 12] == lo, "slot %d: the tie (%d, %d) went to row %d" % (k, lo, hi, rec[k, 12])
        assert got["mask"][k, p_lo] == 1 and got["mask"][k, p_hi] == 0 and got["mask"][k].sum() == 39 == rec[k, 4]
    k = len(expect)
    ang = np.degrees(np.arccos(np.clip(-sc["normals"][0, 2, band].astype(np.float64), -1, 1)))
    assert np.array_equal(got["mask"][k, band], (ang < 20).astype(np.uint8)) and got["mask"][k].sum() == 1 + 24 + 1 == got["counts"][k, 0] == rec[k, 4]
    assert np.abs(np.abs(ang[1:17] - 20) - 0.01).max() < 1e-4                                # the designed pixels are where they should be
    assert got["counts"][k + 1, :3].tolist() == [30, 30, 30] and rec[k + 1, 12] == 0 and rec[k + 1, 5] == 0.0 and rec[k + 1, 6] == 1
    assert np.abs(rec[k + 1, 0:3] - want["rec"][k + 1, 0:3]).max() <= 1e-6
    assert not got["counts"][k + 2].any() and not got["mask"][k + 2].any() and rec[k + 2, 12] == 0 and rec[k + 2, 4] == 0 and rec[k + 2, 6] == 0
    assert got["counts"][k + 3, 0] == 1 and got["mask"][k + 3].sum() == 1 and rec[k + 3, 5] == 0.0 and rec[k + 3, 6] == 1
    assert np.array_equal(rec[:, [4, 6, 12]], want["rec"][:, [4, 6, 12]].astype(F32))
    for j in range(sc["slots"].shape[0]):
        assert rec[j, 4] == got["counts"][j, int(rec[j, 12])] == got["mask"][j].sum()
        assert not got["mask"][j, ids[sc["slots"][j, 0]] != sc["slots"][j, 1]].any()


# ======================================================================================================================================
# 2. vidc_plane_offset / vidc_plane_offset_dense -> vidc_plane_project_depth -> vidc_plane_finalize
# ======================================================================================================================================
@gpu
@pytest.mark.parametrize("H,W", SMALL, ids=IDS)
def test_offset_exact(H, W):
    """n_pts = 0, 1, 2, 299, 300, 301 (as far as the class has inliers), everything exact: first pass (301 points: rec[10] = -1, rec[7] =
    301, rec[6] = rec[9] = 0, the flagged word of `info`), a second pass with a wrong dense_n (flagged again), one with the right dense_n
    (the reference's result; dense_n = 0 for the ordinary slots).  dense_dots[slot][0..n_pts) is the row-major list of the plane's dots:
    the points lie in several sixteenths of the map, in several 256-entry passes of the sparse list and across its wave boundaries; sparse
    points on the background, on other classes and on the class's non-inliers are not in it.  rec[8] is the mean depth.  Image 1 of
    (16, 16) has no sparse depth; image 1 of (7, 9) is background."""
    sc = _exact_scene(H, W)
    dense, first = _dense_for(sc)
    got = _run(sc)
    _compare(sc, got, first)
    if H * W >= 1024:
        k = SLOT_ORDER.index((0, 7))
        assert dense["n_pts"] == {k: 301} and got["rec"][k, [6, 7, 9, 10]].tolist() == [0, 301, 0, -1] and got["info"][-1] == 1
        assert (sc["depth"][0] > 0).sum() > 2 * CH
        _compare(sc, _run(sc, dense, dense_n={k: 300}), first)                               # drawn for another n_pts: flagged again
        pts = np.flatnonzero(first["mask"][k] & (sc["depth"][0] > 0))
        assert np.unique(pts // (-(-H * W // 4096) * 256)).size >= 6
    else:
        assert not dense and got["info"][-1] == 0
    want = _ref_chain(sc, dense)
    got = _run(sc, dense)
    _compare(sc, got, want)
    assert (want["rec"][:, 10] == 1).sum() >= 2 and got["info"][-1] == 0
    n_pts = sorted(want["rec"][:, 7].astype(int).tolist())
    assert n_pts == ([0, 1, 2, 299, 300, 301] if H * W >= 1024 else n_pts) and len(n_pts) == (3 if H * W == 63 else 6)


@gpu
def test_offset_ties_and_the_distance_threshold():
    """Two clusters of equal size: the one that owns the first point in row-major order wins, and moving that point moves the winner.
    0.2f - 0.1f == 0.1f is NOT within 0.1 (one inlier, offset 0.1f); nextafter(0.2f, 0) is (two inliers) -- in the ordinary branch with
    two points, and in the second pass's branch with the pair among 301."""
    for tie, lead in (("a", 1.0), ("b", 1.5)):
        sc = _exact_scene(37, 53, tie)
        got, want = _run(sc, {}), _ref_chain(sc)
        _compare(sc, got, want)
        k = SLOT_ORDER.index((0, 255))
        n = int(want["rec"][k, 7])
        assert n >= 100 and got["rec"][k, 9] == n // 2 and lead <= got["rec"][k, 3] < lead + 0.1
        assert np.floor(-got["dots"][k, [0, n - 1]] * 2).tolist() == [2 * lead, 5 - 2 * lead]
    sc = dict(_exact_scene(16, 16))
    k = SLOT_ORDER.index((0, 7))
    pix = np.flatnonzero(_ref_chain(sc)["mask"][k])
    pix = pix[sc["homo"][0, pix, 2] == 1.0][[0, -1]]
    for second, n_inl, off in ((F32(0.2), 1, F32(0.1)), (np.nextafter(F32(0.2), F32(0)), 2, (F32(0.1) + np.nextafter(F32(0.2), F32(0))) / F32(2))):
        depth = np.zeros_like(sc["depth"])
        depth[0, pix] = F32(0.1), second
        got = _run(sc, {}, depth=depth)
        _compare(sc, got, _ref_chain(sc, depth=depth), depth=depth)
        assert got["rec"][k, [7, 9]].tolist() == [2, n_inl] and got["rec"][k, 3] == off, got["rec"][k]
    # the same pair in the second pass's branch: 150 points in [0.02, 0.093] and 0.1f count 151 whichever of them is the hypothesis; 0.2f
    # joins 0.1f's inliers only when it lies within 0.1 of it, and 0.1f then wins alone with 152 (149 points at 5 m are the rest)
    sc = dict(_exact_scene(37, 53))
    pix = np.flatnonzero(_ref_chain(sc)["mask"][k])[:301]
    ranks = np.random.RandomState(8).permutation(300).astype(np.int32)               # every point but the last one, 0.1f among them
    for second, n_inl in ((F32(0.2), 151), (np.nextafter(F32(0.2), F32(0)), 152)):
        t = np.concatenate([(82 + 2 * np.arange(150)) / 4096.0, [F32(0.1), second], 5 + np.arange(149) / 4096.0]).astype(F32)
        depth = np.zeros_like(sc["depth"])
        depth[0, pix] = t / sc["homo"][0, pix, 2]
        dense = {k: ranks, "n_pts": {k: 301}}
        got, want = _run(sc, dense, depth=depth), _ref_chain(sc, dense, depth=depth)
        assert np.array_equal(got["dots"][k, :301], -t) and got["rec"][k, [6, 7, 9, 10]].tolist() == [1, 301, n_inl, 1] == want["rec"][k, [6, 7, 9, 10]].tolist()
        assert abs(got["rec"][k, 3] - t[:n_inl].astype(np.float64).mean()) <= 1e-6 >= abs(want["rec"][k, 3] - got["rec"][k, 3])


@gpu
@pytest.mark.parametrize("H,W", SMALL, ids=IDS)
def test_chain_noisy(H, W):
    """The five entries on a margin-checked noisy scene, a dense second pass included where the first pass flags a slot."""
    sc = _noisy_scene(H, W)
    dense, first = _dense_for(sc)
    _compare(sc, _run(sc), first)
    if dense:
        _compare(sc, _run(sc, dense), _ref_chain(sc, dense))
    assert bool(dense) == (H * W >= 1024)


@gpu
@pytest.mark.parametrize("H,W", [(16, 16), (65, 64)], ids=["16x16", "65x64"])
def test_misaligned_depth_equals_aligned(H, W):
    """HW % 4 == 0 with the depth pointer one float into its allocation (the list kernel's scalar path): bit for bit the aligned run."""
    for sc in (_exact_scene(H, W), _noisy_scene(H, W)):
        dense, _ = _dense_for(sc)
        a, m = _run(sc, dense), _run(sc, dense, shift=1)
        for key in ("mask", "counts", "rec", "pd", "info", "dots"):
            assert np.array_equal(_bits(a[key]), _bits(m[key])), key
        _compare(sc, m, _ref_chain(sc, dense))


# ======================================================================================================================================
# 3. vidc_plane_project_depth on hand-made records and masks
# ======================================================================================================================================
UP = lambda v: np.nextafter(F32(v), F32(np.inf))                   # noqa: E731
# name: (n pixels, offset, mean depth, rec[6], rec[9], {pixel: z}, valid, n projected); every other z is 1, n_bar = (0, 0, -1): value = offset / z
PROJECT = {
    "rejected": (20, 1.0, 1.0, 0, 5, {}, None, None),
    "no_offset_inliers": (20, 1.0, 1.0, 1, 0, {}, None, None),
    "dot_on_threshold": (20, 0.002, 1.0, 1, 5, {3: F32(1e-3), 4: UP(1e-3), 5: -F32(1e-3)}, 1, 18),
    "all_excluded": (20, 1.0, 1.0, 1, 5, {i: F32(1e-3) for i in range(20)}, 1, 0),
    "one_of_20_big": (20, 1.0, 0.25, 1, 5, {7: 0.25}, 1, 20),
    "one_of_19_big": (19, 1.0, 0.25, 1, 5, {7: 0.25}, 0, 19),
    "exactly_10x_mean": (19, 1.25, 0.25, 1, 5, {7: 0.5}, 1, 19),
    "exactly_10m": (20, 1.25, 2.0, 1, 5, {0: 0.125}, 1, 20),
    "above_10m": (20, UP(1.25), 2.0, 1, 5, {0: 0.125}, 0, 20),
    "one_negative": (20, 1.0, 1.0, 1, 5, {19: -1.0}, 0, 20),
    "ordinary_at_the_end": (20, 1.5, 1.0, 1, 5, {1: 2.0}, 1, 20),
}


@gpu
@pytest.mark.parametrize("H,W", [(7, 9), (37, 53)], ids=["7x9", "37x53"])
def test_project_depth(H, W):
    HW = H * W
    names = sorted(PROJECT) if HW > 1000 else ["dot_on_threshold", "ordinary_at_the_end", "one_negative"]
    n = len(names)
    L = _L()
    slots = np.asarray([(k % 2, (1, 7, 255)[k % 3], 0, 1) for k in range(n)], np.int32)
    homo, mask, rec = np.zeros((2, HW, 3), F32), np.zeros((n, HW), np.uint8), np.zeros((n, REC), F32)
    homo[:, :, 2] = 1
    want = (100 + np.arange(2 * HW, dtype=F32)).reshape(2, HW)
    prefill = want.copy()
    for k, name in enumerate(names):
        npx, off, mean, r6, r9, zs, valid, nproj = PROJECT[name]
        b = k % 2
        px = (HW - 20 if name == "ordinary_at_the_end" else 3 + 20 * (k // 2)) + np.arange(npx)
        for i, z in zs.items():
            homo[b, px[i], 2] = z
        mask[k, px] = 1
        rec[k, 0:3], rec[k, 3], rec[k, 6], rec[k, 8], rec[k, 9], rec[k, 10:12] = (0, 0, -1), off, r6, mean, r9, (7, 7)
        if valid:
            z = homo[b, px, 2]
            ok = np.abs(z) > F32(1e-3)
            want[b, px[ok]] = -F32(off) / (z[ok] * F32(-1))
            assert ok.sum() == nproj
    d_homo, d_slots, d_mask = _dev(homo), _dev(slots), _dev(mask)
    scratch = _Out((L.lib().vidc_plane_scratch_bytes(n, 2, HW),), torch.uint8, 0xFF)
    d_rec, pd = _Out((n, REC), torch.float32, 0.0), _Out((2, HW), torch.float32, 0.0)
    d_rec.t.copy_(_dev(rec))
    pd.t.copy_(_dev(prefill))
    L.check(L.lib().vidc_plane_project_depth(L.ptr(d_homo), L.ptr(d_slots), n, L.ptr(d_mask), HW, scratch.ptr(), d_rec.ptr(), pd.ptr(), L.current_stream()),
            "project_depth")
    torch.cuda.synchronize()
    scratch.np()
    got_rec, got = d_rec.np(), pd.np()
    for k, name in enumerate(names):
        valid, nproj = PROJECT[name][6:8]
        assert got_rec[k, 10:12].tolist() == ([7, 7] if valid is None else [valid, nproj]), (name, got_rec[k])
        b = k % 2
        px = np.flatnonzero(mask[k])
        assert np.array_equal(_bits(got[b, px]), _bits(want[b, px])), (name, got[b, px], want[b, px])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(np.delete(got_rec, [10, 11], 1), np.delete(rec, [10, 11], 1))


# ======================================================================================================================================
# 4. vidc_plane_finalize
# ======================================================================================================================================
@gpu
@pytest.mark.parametrize("n_slots", [0, 5])
@pytest.mark.parametrize("H,W", SMALL, ids=IDS)
def test_finalize(H, W, n_slots):
    """Sparse depths (> 0 only: not 0, -0, negative) override; per-chunk counts of plane_depth > 0 with a partial last chunk (negative and
    NaN plane depths are not counted); the number of slots whose rec[10] is negative; n_slots = 0 with records = NULL."""
    HW = H * W
    rng = np.random.RandomState(HW)
    L = _L()
    pick = lambda vals, p: rng.choice(np.asarray(vals, F32), size=(2, HW), p=p)      # noqa: E731
    depth = pick([0.0, -0.0, -1.0, 1.5, 2.5], [0.5, 0.1, 0.1, 0.2, 0.1])
    pd0 = pick([0.0, -3.0, np.nan, 0.75, 4.0, 1e-30], [0.3, 0.1, 0.1, 0.2, 0.2, 0.1])
    depth[1, -1], pd0[1, -1], depth[0, 0], pd0[0, 0] = 0.0, 0.75, 0.0, np.nan
    rec = rng.uniform(0, 1, (5, REC)).astype(F32)
    rec[:, 10] = [1, -1, 0, -1, -0.0]
    want = np.where(depth > 0, depth, pd0)
    nc = -(-HW // CH)
    gt = np.zeros((2, nc * CH), bool)
    gt[:, :HW] = want > 0
    info_want = np.concatenate([gt.reshape(2, nc, CH).sum(2).reshape(-1), [2 if n_slots else 0]])
    d_depth, d_rec = _dev(depth), _dev(rec)
    pd, info = _Out((2, HW), torch.float32, 0.0), _Out((L.lib().vidc_plane_info_count(2, HW),), torch.int32, -77)
    pd.t.copy_(_dev(pd0))
    assert info.t.numel() == 2 * nc + 1
    L.check(L.lib().vidc_plane_finalize(L.ptr(d_depth), pd.ptr(), 2, HW, L.ptr(d_rec) if n_slots else None, n_slots, info.ptr(), L.current_stream()), "finalize")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pd.np()), _bits(want))
    assert np.array_equal(info.np(), info_want), (info.np(), info_want)


# ======================================================================================================================================
# 5. vidc_enrich_scatter / vidc_enrich_scatter_from
# ======================================================================================================================================
def _enrich_ref(pd, sparse, subs):
    """O.enrich_sparse_depth with the draws given: nz = flatnonzero(pd > 0); out[nz[sub]] = pd[nz[sub]]."""
    out = sparse.copy()
    for b, sub in enumerate(subs):
        nz = np.flatnonzero(pd[b] > 0)
        out[b, nz[sub]] = pd[b, nz[sub]]
    return out


def _enrich_case(HW, variant, rng):
    """plane depths (40 % positive, negatives and NaN among the rest, positive on both sides of every wave and chunk boundary) and the draws."""
    pd = rng.choice(np.asarray([0.0, -2.0, np.nan, 1.0], F32), size=(2, HW), p=[0.4, 0.1, 0.1, 0.4]) * rng.uniform(1, 2, (2, HW)).astype(F32)
    edges = np.asarray([p for p in (63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 1791, 1792, HW - 1) if p < HW])
    pd[:, edges] = 3.0 + edges.astype(F32)
    if variant == "one_candidate":
        pd = np.where(pd > 0, F32(-1.0), pd)
        pd[0, HW - 1], pd[1, 0] = 9.0, 8.0
    subs = []
    for b in range(2):
        nz = np.flatnonzero(pd[b] > 0)
        if variant in ("all", "one_candidate"):
            sub = np.arange(nz.size)
        else:
            sub = np.unique(np.concatenate([[0, nz.size - 1], np.searchsorted(nz, edges), rng.randint(0, nz.size, 10)]))
        subs.append(sub.astype(np.int32))
    if variant.startswith("no_draw_"):
        subs[int(variant[-1])] = np.zeros(0, np.int32)
    return pd, subs


@gpu
@pytest.mark.parametrize("variant", ["edges", "all", "one_candidate", "no_draw_0", "no_draw_1"])
@pytest.mark.parametrize("HW", [63, 1961, 4160])
def test_enrich_scatter(HW, variant):
    """Both variants against the three-line restatement: draws that hit the first and the last non-zero and the non-zeros on both sides of
    wave and chunk boundaries, one candidate, every candidate drawn, an image without a draw (_from: a plain copy; the other variant: the
    pre-fill stays).  Pixels not drawn keep the pre-fill in the variant without the fused clone."""
    L = _L()
    rng = np.random.RandomState(HW + len(variant))
    pd, subs = _enrich_case(HW, variant, rng)
    sparse = rng.choice(np.asarray([0.0, 1.25], F32), size=(2, HW), p=[0.8, 0.2])
    nc = -(-HW // CH)
    gt = np.zeros((2, nc * CH), np.int64)
    gt[:, :HW] = pd > 0
    chunks = gt.reshape(2, nc, CH).sum(2)
    base = (np.cumsum(chunks, 1) - chunks).astype(np.int32)
    sub = np.concatenate(subs + [np.zeros(1, np.int32)])           # (never empty: the entry refuses a null pointer)
    offs = np.asarray([0, subs[0].size, subs[0].size + subs[1].size], np.int32)
    d_pd, d_sp, d_sub, d_offs, d_base = _dev(pd), _dev(sparse), _dev(sub), _dev(offs), _dev(base)
    st = L.current_stream()
    out_from, out = _Out((2, HW), torch.float32, float("nan")), _Out((2, HW), torch.float32, float("nan"))
    L.check(L.lib().vidc_enrich_scatter_from(L.ptr(d_pd), L.ptr(d_sp), L.ptr(d_sub), L.ptr(d_offs), L.ptr(d_base), 2, HW, out_from.ptr(), st), "scatter_from")
    L.check(L.lib().vidc_enrich_scatter(L.ptr(d_pd), L.ptr(d_sub), L.ptr(d_offs), L.ptr(d_base), 2, HW, out.ptr(), st), "scatter")
    torch.cuda.synchronize()
    want = _enrich_ref(pd, sparse, subs)
    assert np.array_equal(_bits(out_from.np()), _bits(want)), np.argwhere(out_from.np() != want)[:4]
    assert np.array_equal(_bits(out.np()), _bits(_enrich_ref(pd, np.full((2, HW), np.nan, F32), subs)))
    if variant.startswith("no_draw_"):
        b = int(variant[-1])
        assert np.isnan(out.np()[b]).all() and np.array_equal(out_from.np()[b], sparse[b]) and not np.isnan(out.np()[1 - b]).all()


# ======================================================================================================================================
# 6. vidc_plane_block
# ======================================================================================================================================
def _same(a, b):
    for key in ("mask", "counts", "rec", "pd", "info", "dots"):
        if a[key] is not None or b[key] is not None:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), key


@gpu
@pytest.mark.parametrize("H,W", [(37, 53), (65, 64)], ids=["37x53", "65x64"])
def test_plane_block_equals_the_five_entries(H, W):
    """Bit for bit, B = 2: first pass without dense_*, the dense second pass, and the n_slots = 0 form (copy + finalize)."""
    for sc in (_noisy_scene(H, W), _exact_scene(H, W)):
        dense, _ = _dense_for(sc)
        assert dense
        _same(_run(sc, block=True), _run(sc))
        blk = _run(sc, dense, block=True)
        _same(blk, _run(sc, dense))
        _compare(sc, blk, _ref_chain(sc, dense))
        none = _run(sc, block=True, n_slots=0)
        _same(none, _run(sc, n_slots=0))
        assert np.array_equal(none["pd"], sc["depth"]) and none["info"][-1] == 0 and none["info"][:-1].sum() == (sc["depth"] > 0).sum()
        assert (none["mask"] == 0xFF).all() and (none["counts"] == -77).all() and np.isnan(none["rec"]).all()


@gpu
def test_plane_block_240x320():
    """The one 240x320 case: the list kernel's 1024-pixel straight loop and the whole block in one call, both passes."""
    sc = _noisy_scene(240, 320, density=(0.02, 0.005))
    dense, first = _dense_for(sc)
    assert dense and (first["rec"][:, 10] >= 0).any()
    _compare(sc, _run(sc, block=True), first)
    _compare(sc, _run(sc, dense, block=True), _ref_chain(sc, dense))


def _oracle_block(sc, seed, goal):
    """O.extract_plane_depth image by image and O.enrich_sparse_depth, with the generators PlaneBlock gets."""
    H, W = sc["H"], sc["W"]
    rng = np.random.RandomState(seed)
    di = torch.stack([O.extract_plane_depth(torch.from_numpy(sc["normals"][b]).view(3, H, W), torch.from_numpy(sc["ids"][b].astype(np.int64)).view(H, W),
                                            torch.from_numpy(sc["depth"][b]).view(H, W), torch.from_numpy(sc["homo"][b]).view(H, W, 3), rng=rng)
                      for b in range(2)])[:, None]
    ds = torch.from_numpy(sc["depth"]).view(2, 1, H, W)
    return di, O.enrich_sparse_depth(ds, di, goal, rng=np.random.RandomState(seed + 1))


PB_SEED, PB_GOAL = 11, 60


@gpu
def test_plane_block_class_against_the_oracle():
    """PlaneBlock with a RandomState at (37, 53), B = 2, on a scene whose margins hold for the rows that generator draws: the set of written
    pixels equals the oracle's, of the plane depth and of the enriched depth; values within the depth bound."""
    from vi_depth_completion_amd import plane
    sc = _noisy_scene(37, 53, drawn=PB_SEED, density=(0.1, 0.1))
    H, W = 37, 53
    want_di, want_en = _oracle_block(sc, PB_SEED, PB_GOAL)
    pb = plane.PlaneBlock()
    ds = _dev(sc["depth"]).view(2, 1, H, W)
    di, info = pb.plane_depth(_dev(sc["normals"]).view(2, 3, H, W), [m.reshape(H, W) for m in sc["ids"]], ds, _dev(sc["homo"]).view(2, H, W, 3),
                              rng=np.random.RandomState(PB_SEED))
    en = pb.enrich(ds, di, info, PB_GOAL, rng=np.random.RandomState(PB_SEED + 1)).cpu()
    di = di.cpu()
    assert torch.equal(di != ds.cpu(), want_di != ds.cpu()) and int((di != ds.cpu()).sum()) > 500
    assert torch.equal(en != ds.cpu(), want_en != ds.cpu()) and int((en != ds.cpu()).sum()) > 50
    bound, _ = _bounds()
    _note("PlaneBlock 37x53 depth", (di - want_di).abs().max(), 2 * bound["depth"])
    assert (di - want_di).abs().max() <= 2 * bound["depth"] and (en - want_en).abs().max() <= 2 * bound["depth"]      # (two fp32 evaluations)


# ======================================================================================================================================
# CPU tests: the restatements against the oracle, the margins of the generated inputs, the host's refusals
# ======================================================================================================================================
def test_fp32_facts_behind_the_designed_inputs():
    assert F32(0.2) - F32(0.1) == F32(0.1) and not abs(F32(0.1) - F32(0.2)) < F32(0.1)
    assert abs(F32(0.1) - np.nextafter(F32(0.2), F32(0))) < F32(0.1)
    t = torch.tensor
    assert not bool(t(1) / 20 > 0.05) and bool(t(1) / 19 > 0.05) and not F32(1) / F32(20) > THR_FRAC and F32(1) / F32(19) > THR_FRAC
    assert not bool(t(1e-3).abs() > 1e-3) and bool(t(float(UP(1e-3))).abs() > 1e-3)
    assert not bool(t(10.0) > O.MAX_DEPTH) and bool(t(float(UP(10.0))) > O.MAX_DEPTH) and UP(1.25) / F32(0.125) == UP(10.0)


@pytest.mark.parametrize("H,W", SMALL, ids=IDS)
def test_restatement_equals_the_oracle_and_margins_hold(H, W):
    """Noisy scenes: no (hypothesis, pixel) angle within 2e-3 degrees of 20, no |hyp + dot| within 1e-6 of 0.1, no |n.homo| within 1e-6 of
    1e-3, every projected value far from 0 / 10 m / 10 x mean, at least 1 degree of mean angle -- and under these the fp32 oracle takes every
    decision like the float64 restatement.  Exact scenes: the restatement equals the oracle bit for bit."""
    for sc in (_noisy_scene(H, W), _exact_scene(H, W)):
        dense, first = _dense_for(sc)
        assert bool(dense) == (H * W >= 1024)
        for dn, want in ((None, first), (dense, _ref_chain(sc, dense))):
            res, pd = _oracle32(sc, dn)
            for k, r in enumerate(res):
                rec = want["rec"][k]
                assert np.array_equal(r["mask"], want["mask"][k].astype(bool)), k
                assert r["n_off"] == rec[9] and (r["valid"] is None or r["valid"] == rec[10])
                if sc["exact"]:
                    assert np.array_equal(r["n_bar"], rec[0:3].astype(F32)) and r["mean_angle"] == 0 and F32(r["offset"]) == F32(rec[3])
            assert np.array_equal(pd != sc["depth"], want["written"])
            if sc["exact"]:
                assert np.array_equal(pd, want["pd"].astype(F32))
            else:
                assert want["m_angle"] >= 2e-3 and want["m_dist"] >= 1e-6 and want["m_dot"] >= 1e-6, (want["m_angle"], want["m_dist"], want["m_dot"])
                acc = want["rec"][:, 6] > 0
                assert (want["rec"][want["rec"][:, 4] > 1, 5] >= 1.0).all() and (want["rec"][:, 5] < 19).all()
                vals = want["pd"][want["written"]]
                assert vals.size == 0 or (vals.min() > 0.5 and vals.max() < 9 and want["rec"][acc & (want["rec"][:, 9] > 0), 8].min() > 1.0)
    bound, dev = _bounds()
    print("fp32 oracle against float64:", dev)
    assert all(v > 0 for v in dev.values()) and bound["n_bar"] < 1e-5 and bound["mean_angle"] < 1e-2 and bound["offset"] < 1e-4 and bound["depth"] < 1e-4


def test_special_and_tie_inputs():
    """The tie clusters are more than 40 degrees apart and count 39 / 39; the band pixels sit 0.01 degrees beside 20 (5x the generator's
    margin, inside the kernel's +-1e-4 cosine band); the exact tie scenes put cluster A / B first and the other one last."""
    sc, expect, band = _special_scene()
    want = _ref_chain(sc)
    assert want["m_angle"] > 9.9e-3
    for k, (lo, hi, _p, _q) in enumerate(expect):
        assert want["rec"][k, 12] == lo and want["counts"][k, lo] == want["counts"][k, hi] == 39 and np.sort(want["counts"][k])[-3] <= 30
    c = -sc["normals"][0, 2, band[1:17]].astype(np.float64)
    assert (np.abs(c - np.cos(np.radians(20))) < 1e-4).all()
    res, _ = _oracle32(sc)
    for k in range(sc["slots"].shape[0]):
        assert np.array_equal(res[k]["mask"], want["mask"][k].astype(bool)), k
    for tie in "ab":
        sc = _exact_scene(37, 53, tie)
        k = SLOT_ORDER.index((0, 255))
        d = _ref_chain(sc)["dots"][k]
        assert (d[0] > -1.25) == (tie == "a") and (d[-1] > -1.25) == (tie == "b") and (d > -1.25).sum() * 2 == d.size


def test_drawn_scene_and_enrichment_restatement():
    """The scene of the PlaneBlock test: the restatement, fed PlaneBlock's draws, writes the pixels O.extract_plane_depth writes, with margins;
    the three-line enrichment restatement equals O.enrich_sparse_depth."""
    sc = _noisy_scene(37, 53, drawn=PB_SEED, density=(0.1, 0.1))
    want = _ref_chain(sc)
    assert want["m_angle"] >= 2e-3 and want["m_dist"] >= 1e-6 and want["m_dot"] >= 1e-6 and want["info"][-1] == 0
    di, en = _oracle_block(sc, PB_SEED, PB_GOAL)
    assert np.array_equal(di.view(2, -1).numpy() != sc["depth"], want["written"]) and np.abs(di.view(2, -1).numpy() - want["pd"]).max() < 1e-4
    trace = []
    O.enrich_sparse_depth(torch.from_numpy(sc["depth"]).view(2, 1, 37, 53), di, PB_GOAL, rng=np.random.RandomState(PB_SEED + 1), trace=trace)
    got = _enrich_ref(di.view(2, -1).numpy(), sc["depth"], [t["sub"] for t in trace])
    assert np.array_equal(got, en.view(2, -1).numpy()) and (got != sc["depth"]).sum() > 50


@pytest.fixture(scope="module")
def lib():
    L = _L()
    L.build()
    return L.lib()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    p, q = 4096, 8192                                              # never dereferenced: every call below is refused first
    null, shape = [], []
    nrm = lambda a, n=1, hw=63: lib.vidc_plane_ransac_normal(a[0], a[1], a[2], n, a[3], hw, a[4], a[5], a[6], None)        # noqa: E731
    null += [nrm([None if i == j else p for i in range(7)]) for j in range(7)]
    shape += [nrm([p] * 7, n, hw) for n, hw in ((0, 63), (-1, 63), (1, 0), (1, -5))]
    off = lambda a, n=1, B=2, hw=63: lib.vidc_plane_offset(a[0], a[1], a[2], n, B, a[3], a[4], hw, a[5], a[6], None)      # noqa: E731
    null += [off([None if i == j else p for i in range(7)]) for j in range(7)]
    shape += [off([p] * 7, n, B, hw) for n, B, hw in ((0, 2, 63), (1, 0, 63), (1, 2, 0))]
    for lone in ((p, None, None), (None, p, None), (None, None, p), (p, p, None)):
        null.append(lib.vidc_plane_offset_dense(p, p, p, 1, 2, p, p, 63, p, p, *lone, None))
    prj = lambda a, n=1, hw=63: lib.vidc_plane_project_depth(a[0], a[1], n, a[2], hw, a[3], a[4], a[5], None)             # noqa: E731
    null += [prj([None if i == j else p for i in range(6)]) for j in range(6)]
    shape += [prj([p] * 6, 0), prj([p] * 6, 1, 0)]
    null += [lib.vidc_plane_finalize(None, p, 2, 63, p, 1, p, None), lib.vidc_plane_finalize(p, None, 2, 63, p, 1, p, None),
             lib.vidc_plane_finalize(p, p, 2, 63, p, 1, None, None), lib.vidc_plane_finalize(p, p, 2, 63, None, 1, p, None)]
    shape += [lib.vidc_plane_finalize(p, p, 0, 63, p, 1, p, None), lib.vidc_plane_finalize(p, p, 2, 0, p, 1, p, None),
              lib.vidc_plane_finalize(p, p, 2, 63, p, -1, p, None)]
    blk = lambda depth, pd, info, n=1, B=2, hw=63: lib.vidc_plane_block(p, p, p, n, p, B, hw, p, depth, p, p, p, p, None, None, None, pd, info, None)      # noqa: E731
    null += [blk(None, p, p), blk(p, None, p), blk(p, p, None)]
    shape += [blk(p, p, p, -1), blk(p, p, p, 1, 0), blk(p, p, p, 1, 2, 0)]
    sc = lambda a, B=2, hw=63: lib.vidc_enrich_scatter(a[0], a[1], a[2], a[3], B, hw, a[4], None)                          # noqa: E731
    scf = lambda a, B=2, hw=63: lib.vidc_enrich_scatter_from(a[0], a[1], a[2], a[3], a[4], B, hw, a[5], None)              # noqa: E731
    null += [sc([None if i == j else p for i in range(5)]) for j in range(5)] + [scf([None if i == j else p for i in range(6)]) for j in range(6)]
    shape += [sc([p] * 5, 0), sc([p] * 5, 2, 0), scf([p] * 5 + [q], 0), scf([p] * 5 + [q], 2, 0), scf([p, q, p, p, p, q])]      # enriched == sparse_depth
    assert null == [ERR_NULL] * len(null), null
    assert shape == [ERR_SHAPE] * len(shape), shape
    assert lib.vidc_plane_info_count(2, 63) == 3 and lib.vidc_plane_info_count(2, 1961) == 17
    assert lib.vidc_plane_scratch_bytes(3, 2, 1961) == 3 * 8 * 9 * 4 + 2 * 1962 * 4 + 256


def test_plane_groups_rejects_ids_the_device_cannot_hold():
    """The device compares uint8 ids: an id above 255 (or below 0) in a wider map would alias another plane or the background there."""
    from vi_depth_completion_amd import plane
    m = np.zeros((4, 5), np.int64)
    m[1, 2], m[3, 3] = 255, 7
    assert [c for c, _ in plane.plane_groups(m)] == [7, 255] == [c for c, _ in plane.plane_groups(m.astype(np.uint8))]
    for bad in (256, 1000, -1):
        m[0, 0] = bad
        with pytest.raises(ValueError):
            plane.plane_groups(m)
        for dt in (np.int32, np.int16, np.float32):
            with pytest.raises(ValueError):
                plane.plane_groups(m.astype(dt))
