"""Training-batch pre-processing (csrc/train_preprocess.hip, ScanNetFramePreprocessor / NYUFramePreprocessor): the device counterpart of
the reference's ScanNetSmallFramesDataset.__getitem__ (dataset.py:95-247) and NYUDataset.__getitem__ (dataset.py:381-438).

CPU: the restatement (tests/train_preprocess_ref.py) against the literal numpy / torch sequences on every byte and every 16-bit value, the
alignment rule, the random-sample draw protocol against numpy itself, the refusals of every new entry.
GPU: every kernel through the C ABI at edge shapes, outputs and scratch owned by the test (pre-filled, a guard region behind each), and
both classes end to end against the restatement's dictionaries.  Everything is compared for equality: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_preprocess_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
ERR_NULL, ERR_SHAPE = -1, -2                                       # include/vidc.h
GUARD = 64
# the SIZES of tests/test_preprocess.py
SIZES = [((480, 640), (240, 320)), ((720, 1280), (240, 320)), ((480, 640), (256, 320)), ((100, 130), (37, 51)), ((60, 80), (60, 80)),
         ((30, 40), (45, 64))]
MODES = (0, 1, 2, 3)


def _L():
    from vi_depth_completion_amd import _lib as L
    return L


def _lib():
    L = _L()
    L.build()
    return L.lib()


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    """Equal shapes, dtypes and bit patterns."""
    g, w = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)) for x in (got, want))
    return tuple(g.shape) == tuple(w.shape) and g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w))


# ======================================================================================================================================
# CPU
# ======================================================================================================================================
def test_byte_expressions_equal_the_literal_sequences_on_all_256_values():
    img3 = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    img3 = np.ascontiguousarray((img3 + np.array([0, 85, 171])) % 256).astype(np.uint8)      # every channel holds every byte
    img1 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for c in range(3):
        assert np.array_equal(np.sort(img3[:, :, c].reshape(-1)), np.arange(256))
    assert _same(R.decode_u8(img3, 0), R.color_literal(img3))
    assert _same(R.decode_u8(img1, 0)[0], R.mask_literal(img1))
    assert _same(R.decode_u8(img3, 1), R.normal_gt_literal(img3))
    assert _same(R.decode_u8(img3, 2), R.predicted_normal_scannet_literal(img3))
    assert _same(R.decode_u8(img3, 3), R.predicted_normal_nyu_literal(img3))


def test_mask_float64_form_equals_fp32_form_on_all_256_values():
    x = np.arange(256, dtype=np.uint8)
    f64 = torch.Tensor(x / 255.0)                                   # dataset.py:129
    f32 = torch.from_numpy(x).float() / 255
    assert f64.dtype == torch.float32 and _same(f64, f32)
    assert np.array_equal((x / 255.0).astype(np.float32), x.astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("divisor", [1000.0, 5000.0])
def test_depth_float64_form_equals_fp32_form_on_all_65536_values(divisor):
    x = np.arange(65536, dtype=np.int64).astype(np.uint16)
    f64 = torch.tensor(x / divisor).float()                         # dataset.py:124-125
    assert _same(f64, R.depth_fp32(x, divisor))
    assert _same(torch.Tensor(x.astype(np.float32)) / divisor, R.depth_fp32(x, divisor))      # dataset.py:405
    if divisor == 1000.0:
        assert _same(R.scannet_depth_literal(x.reshape(256, 256))[0], R.depth_fp32(x, 1000.0).view(256, 256))


def test_alignment_rule_on_both_sides_of_its_thresholds():
    from vi_depth_completion_amd import preprocess
    up = torch.tensor([0.0, 1.0, 0.0])
    cases = []
    for s in (0.9e-3, 0.99e-3, 1.0e-3, 1.01e-3, 1.1e-3):           # psi = s^2 around 1e-6
        cases += [(0.5, s, 0.0), (0.5, 0.0, s), (0.5, -s, 0.0)]
    for c in (0.29, 0.2999, 0.3, 0.3001, 0.31, -0.5, 1.0):         # cos(pitch) = g1 / |(g1, g2)| around 0.3
        sn = float(np.sqrt(1.0 - c * c))
        cases += [(0.1, c, sn), (0.1, c, -sn), (0.0, 2 * c, 2 * sn)]
    seen = set()
    for g in cases:
        gt = torch.tensor(np.asarray(g, dtype=np.float64), dtype=torch.float)
        want = R.compute_alignment_tensor(gt)
        got_g, got_a = preprocess.scannet_gravity_and_alignment(g)
        assert _same(got_g, gt) and _same(got_a, want), g
        psi = float(gt[1] * gt[1] + gt[2] * gt[2])
        seen.add("small" if psi < 1e-6 else ("up" if torch.equal(want, up) else "gravity"))
        if psi >= 1e-6:
            assert torch.equal(want, up) == bool(torch.cos(torch.atan2(gt[2], gt[1])) > 0.3)
    assert seen == {"small", "up", "gravity"}
    # the float32 neighbours of the two thresholds themselves
    for psi32 in (np.nextafter(np.float32(1e-6), np.float32(0)), np.float32(1e-6), np.nextafter(np.float32(1e-6), np.float32(1))):
        g = (0.25, float(np.sqrt(np.float64(psi32))), 0.0)
        assert _same(preprocess.scannet_gravity_and_alignment(g)[1], R.compute_alignment_tensor(torch.tensor(g, dtype=torch.float)))


def _draws_reference(counts, num_points, rng):
    """dataset.py:193-200 image by image: what is drawn, and from what."""
    out = []
    for count, n in zip(counts, num_points):
        out.append(None if n >= count else rng.permutation(count)[0:n])
    return out


def _check_draws(counts, num_points, make_rng):
    from vi_depth_completion_amd import preprocess
    a, b = make_rng(), make_rng()
    want = _draws_reference(counts, num_points, a)
    perm, sel_off, nsel = preprocess.draw_sparse_sample(counts, num_points, b)
    assert perm.dtype == np.int32 and sel_off.dtype == np.int32 and nsel.dtype == np.int32
    for i, w in enumerate(want):
        if w is None:
            assert nsel[i] == -1
        else:
            assert nsel[i] == len(w) and np.array_equal(perm[sel_off[i]:sel_off[i] + nsel[i]], w), i
    assert len(perm) == sum(len(w) for w in want if w is not None)
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and sa[2] == sb[2] and np.array_equal(sa[1], sb[1]) and sa[3:] == sb[3:]      # the generator state, word by word
    assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)                                                # ... and the next draw


def test_random_sample_draw_protocol_against_numpy():
    count = 700                                                     # beyond one 624-word refill of the MT19937 state
    for seed in (0, 7):
        mk = lambda: np.random.RandomState(seed)                    # noqa: E731
        # a batch of three, the middle image a clone (nothing drawn for it)
        _check_draws([count, 50, 1961], [300, 50, 17], mk)
        for n in (0, 1, count - 1, count, count + 1):
            _check_draws([count], [n], mk)
            _check_draws([31, count, 5], [4, n, 0], mk)
        _check_draws([0, 0, 3], [0, 1, 2], mk)                      # an all-zero ground truth: 0 >= 0 is the clone
    # np.random itself (the module's global legacy generator)
    saved = np.random.get_state()
    try:
        from vi_depth_completion_amd import preprocess
        np.random.seed(11)
        want = _draws_reference([count, 10, 90], [12, 10, 0], np.random)
        st_want = np.random.get_state()
        nxt_want = np.random.randint(0, 1 << 30)
        np.random.seed(11)
        perm, sel_off, nsel = preprocess.draw_sparse_sample([count, 10, 90], [12, 10, 0])      # rng defaults to np.random
        st_got = np.random.get_state()
        assert nsel.tolist() == [12, -1, 0] and sel_off.tolist() == [0, 12, 12] and np.array_equal(perm, want[0]) and len(want[2]) == 0
        assert st_want[2] == st_got[2] and np.array_equal(st_want[1], st_got[1])
        assert np.random.randint(0, 1 << 30) == nxt_want
    finally:
        np.random.set_state(saved)
    # a generator that is not the legacy one goes through its own permutation()
    ga, gb = np.random.default_rng(3), np.random.default_rng(3)
    from vi_depth_completion_amd import preprocess
    perm, sel_off, nsel = preprocess.draw_sparse_sample([40, 9], [5, 9], gb)
    assert np.array_equal(perm, ga.permutation(40)[0:5]) and nsel.tolist() == [5, -1]
    assert ga.integers(1 << 30) == gb.integers(1 << 30)


def test_legacy_permutation_of_an_int_equals_permutation_of_the_range():
    """dataset.py:200 draws permutation(n); plane._LegacyStream replays permutation(np.r_[0:n]) (main.py:43): the same values, the same
    state afterwards."""
    for seed in (0, 5):
        for n in (0, 1, 2, 17, 623, 624, 625, 4097):
            a, b = np.random.RandomState(seed), np.random.RandomState(seed)
            assert np.array_equal(a.permutation(n), b.permutation(np.r_[0:n]))
            sa, sb = a.get_state(), b.get_state()
            assert sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def test_num_points_of_the_empty_file_and_the_failed_read():
    """dataset.py:183-193: np.atleast_2d of an empty file's loadtxt has one row, the failed read's np.zeros((0, 4)) none; neither holds a
    track for the sparse map."""
    from vi_depth_completion_amd import preprocess
    empty_file, failed = np.zeros((0,)), np.zeros((0, 4))
    assert [np.atleast_2d(np.asarray(t)).shape[0] for t in (empty_file, failed, np.zeros(4), np.zeros((5, 4)))] == [1, 0, 1, 5]
    rows, offs = preprocess.track_rows([empty_file, failed, np.arange(4.0), np.ones((5, 4)), np.ones((2, 3))])
    assert offs.tolist() == [0, 0, 0, 1, 6, 8] and rows.shape == (8, 4) and rows[6:, 3].tolist() == [0.0, 0.0]


def test_refusals_without_a_gpu():
    lib = _lib()
    p = 4096                                                         # a non-NULL value that no refused call may touch
    # (a)
    assert lib.vidc_u8_decode_chw(None, p, 1, 4, 4, 3, 0, None) == ERR_NULL
    assert lib.vidc_u8_decode_chw(p, None, 1, 4, 4, 3, 0, None) == ERR_NULL
    for B, H, W, Cc, mode in ((0, 4, 4, 3, 0), (1, 0, 4, 3, 0), (1, 4, 0, 3, 0), (1, 4, 4, 2, 0), (1, 4, 4, 4, 0), (1, 4, 4, 3, 4), (1, 4, 4, 3, -1),
                              (1, 65536, 65536, 1, 0)):
        assert lib.vidc_u8_decode_chw(p, p, B, H, W, Cc, mode, None) == ERR_SHAPE, (B, H, W, Cc, mode)
    assert b"vidc_u8_decode_chw" in lib.vidc_last_error()
    # (b)
    assert lib.vidc_rasterize_pixel_tracks(p, None, 1, 1, 2.0, None, p, 4, 4, p, None) == ERR_NULL
    assert lib.vidc_rasterize_pixel_tracks(p, p, 1, 1, 2.0, None, None, 4, 4, p, None) == ERR_NULL
    assert lib.vidc_rasterize_pixel_tracks(p, p, 1, 1, 2.0, None, p, 4, 4, None, None) == ERR_NULL
    assert lib.vidc_rasterize_pixel_tracks(None, p, 1, 1, 2.0, None, p, 4, 4, p, None) == ERR_NULL      # tracks may be NULL only with 0 tracks
    for n, B, div, H, W in ((-1, 1, 2.0, 4, 4), (1, 0, 2.0, 4, 4), (1, 1, 0.0, 4, 4), (1, 1, float("nan"), 4, 4), (1, 1, 2.0, 0, 4), (1, 1, 2.0, 4, 0),
                            (1, 4, 2.0, 32768, 32768)):
        assert lib.vidc_rasterize_pixel_tracks(p, p, n, B, div, None, p, H, W, p, None) == ERR_SHAPE, (n, B, div, H, W)
    assert lib.vidc_rasterize_pixel_tracks_scratch_bytes(2, 5, 7) == 2 * 5 * 7 * 4 and lib.vidc_rasterize_pixel_tracks_scratch_bytes(0, 5, 7) == 0
    # (c)
    for args in ((None, 1, 8, p, p, p), (p, 1, 8, None, p, p), (p, 1, 8, p, None, p), (p, 1, 8, p, p, None)):
        assert lib.vidc_nonzero_compact(*args, None) == ERR_NULL
    for B, HW in ((0, 8), (1, 0), (-1, 8), (1, -8), (1, 0x7fffffff)):
        assert lib.vidc_nonzero_compact(p, B, HW, p, p, p, None) == ERR_SHAPE, (B, HW)
    ck = _L().NONZERO_CHUNK
    assert [lib.vidc_nonzero_compact_scratch_bytes(2, n) for n in (1, ck, ck + 1, 76800)] == [8, 8, 16, 8 * 75] and lib.vidc_nonzero_compact_scratch_bytes(2, 0) == 0
    # (d)
    for i in range(6):
        a = [p, p, p, p, p, 1, 1, 8, p]
        a[i if i < 5 else 8] = None
        assert lib.vidc_sparse_sample_scatter(*a, None) == ERR_NULL, i
    for max_sel, B, HW in ((-1, 1, 8), (9, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert lib.vidc_sparse_sample_scatter(p, p, p, p, p, max_sel, B, HW, p, None) == ERR_SHAPE, (max_sel, B, HW)
    # (e)
    for i in (0, 1, 7, 8):
        a = [p, p, 1, 4, 4, 2, 2, p, p, 5000.0, 0.1, 7.0]
        a[i] = None
        assert lib.vidc_resize_nearest_u16_depth_range(*a, None) == ERR_NULL, i
    for B, H, W, Ho, Wo, div, lo, hi in ((0, 4, 4, 2, 2, 5000.0, 0.1, 7.0), (1, 0, 4, 2, 2, 5000.0, 0.1, 7.0), (1, 4, 4, 0, 2, 5000.0, 0.1, 7.0),
                                         (1, 4, 4, 2, 0, 5000.0, 0.1, 7.0), (1, 4, 4, 2, 2, 0.0, 0.1, 7.0), (1, 4, 4, 2, 2, 5000.0, 7.0, 0.1)):
        assert lib.vidc_resize_nearest_u16_depth_range(p, p, B, H, W, Ho, Wo, p, p, div, lo, hi, None) == ERR_SHAPE
    assert b"vidc_resize_nearest_u16_depth_range" in lib.vidc_last_error()


def test_classes_need_a_gpu_and_have_no_cpu_path():
    from vi_depth_completion_amd import preprocess
    assert issubclass(preprocess.ScanNetFramePreprocessor, preprocess.FramePreprocessor)
    assert issubclass(preprocess.NYUFramePreprocessor, preprocess.FramePreprocessor)
    if not torch.cuda.is_available():
        for cls in (preprocess.ScanNetFramePreprocessor, preprocess.NYUFramePreprocessor):
            with pytest.raises(RuntimeError):
                cls("cuda")


# ======================================================================================================================================
# GPU
# ======================================================================================================================================
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Out:
    """A device buffer pre-filled with `fill`, GUARD untouchable elements behind it (tests/test_metrics_kernels.py)."""

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


def _scratch(nbytes):
    """Exactly `nbytes` of scratch (whole int32 words) with a guard behind it."""
    assert nbytes % 4 == 0
    return _Out((nbytes // 4,), torch.int32, 0x5A5A5A5A)


def _stream():
    return _L().current_stream()


# ---- (a) vidc_u8_decode_chw ----------------------------------------------------------------------------------------------------------
def _byte_images(B, H, W, Cc, start):
    """Images that walk through all 256 byte values, starting at `start`, in an order that differs between the channels."""
    n = B * H * W * Cc
    a = (np.arange(n, dtype=np.int64) * 37 + start) % 256            # 37 is odd: 256 consecutive elements hold every value
    return a.astype(np.uint8).reshape((B, H, W, Cc))


@gpu
@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (37, 53), (240, 320)])
@pytest.mark.parametrize("mode", MODES)
def test_hip_u8_decode(mode, hw):
    lib = _lib()
    H, W = hw
    B = 2
    for Cc in (1, 3):
        starts = range(0, 256, 64) if B * H * W * Cc < 256 else (0,)      # the 5x7 maps see every byte over four launches
        seen = np.zeros(256, bool)
        for start in starts:
            img = _byte_images(B, H, W, Cc, start)
            seen[np.unique(img)] = True
            want = torch.stack([R.decode_u8(img[b], mode) for b in range(B)]).numpy()
            # aligned base (16-byte loads where H*W allows), and the same bytes one byte further on: the element-wise path
            for shift in (0, 1):
                buf = torch.zeros(img.size + 16, dtype=torch.uint8, device=DEV)
                assert buf.data_ptr() % 16 == 0
                buf[shift:shift + img.size] = _dev(img.reshape(-1))
                out = _Out((B, Cc, H, W), torch.float32, -7.0)
                assert lib.vidc_u8_decode_chw(buf.data_ptr() + shift, out.ptr(), B, H, W, Cc, mode, _stream()) == 0
                assert np.array_equal(_bits(out.np()), _bits(want)), (Cc, start, shift)
        assert seen.all()
    if hw == (16, 16) and mode == 0:
        # an output base that is 4- but not 16-byte aligned: the element-wise path again
        img = _byte_images(B, H, W, 3, 5)
        out = _Out((B * 3 * H * W + 1,), torch.float32, -7.0)
        src = _dev(img)
        assert lib.vidc_u8_decode_chw(src.data_ptr(), out.ptr() + 4, B, H, W, 3, mode, _stream()) == 0
        got = out.np()
        assert got[0] == -7.0 and np.array_equal(_bits(got[1:]), _bits(torch.stack([R.decode_u8(img[b], 0) for b in range(B)]).numpy().reshape(-1)))


# ---- (b) vidc_rasterize_pixel_tracks -------------------------------------------------------------------------------------------------
def _tracks(n, H, W, seed, edge=False):
    rng = np.random.RandomState(seed)
    t = np.stack([np.arange(n, dtype=np.float64), rng.uniform(-4.0, 2 * W + 4.0, n), rng.uniform(-4.0, 2 * H + 4.0, n), rng.uniform(0.5, 5.0, n)], axis=1)
    if edge:
        assert n >= 40
        xs = [-1.0, -2.0, 2 * W - 0.5, 2.0 * W, float("nan"), 1e300, -1e300, float("inf"), 4294967296.0 + 2.0, -0.0]
        for k, x in enumerate(xs):
            t[2 * k, 1], t[2 * k, 2] = x, 3.0                        # in x, y on row 1
            t[2 * k + 1, 1], t[2 * k + 1, 2] = 3.0, (x if x not in (2 * W - 0.5, 2.0 * W) else x - 2 * W + 2 * H)     # in y, x on column 1
    return t


def _run_tracks(lib, tables, H, W, gt):
    B = len(tables)
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum([len(t) for t in tables])
    n = int(offs[-1])
    tr = _dev(np.concatenate(tables)) if n else None
    out = _Out((B, H, W), torch.float32, -7.0)
    nb = lib.vidc_rasterize_pixel_tracks_scratch_bytes(B, H, W)
    assert nb == B * H * W * 4
    sc = _scratch(nb)
    g = _dev(gt) if gt is not None else None
    assert lib.vidc_rasterize_pixel_tracks(None if tr is None else tr.data_ptr(), _dev(offs).data_ptr(), n, B, 2.0, None if g is None else g.data_ptr(),
                                           out.ptr(), H, W, sc.ptr(), _stream()) == 0
    sc.np()
    return out.np()


@gpu
@pytest.mark.parametrize("case", ["empty", "one", "same_pixel", "edges173", "crowd5000"])
def test_hip_rasterize_pixel_tracks(case):
    lib = _lib()
    H, W = (5, 7) if case in ("empty", "one", "crowd5000") else (37, 53)
    if case == "empty":
        tables = [np.zeros((0, 4)), np.zeros((0, 4))]
    elif case == "one":
        tables = [np.zeros((0, 4)), np.array([[0, 6.9, 4.2, 1.5]])]
    elif case == "same_pixel":
        tables = [np.array([[0, 10.0, 8.0, 1.0], [1, 11.9, 9.9, 2.0]]), _tracks(3, H, W, 1)]      # (5, 4) twice: the later one stays
    elif case == "edges173":
        tables = [_tracks(173, H, W, 2, edge=True), _tracks(1, H, W, 3)]
    else:
        tables = [_tracks(5000, H, W, 4), _tracks(173, H, W, 5, edge=True)]                       # ~100 tracks per pixel
    gt = np.random.RandomState(9).uniform(0.0, 6.0, (len(tables), H, W)).astype(np.float32)
    for g in (None, gt):
        got = _run_tracks(lib, tables, H, W, g)
        for b, t in enumerate(tables):
            want = R.pixel_tracks(t, H, W, None if g is None else torch.from_numpy(g[b])).numpy()[0]
            assert np.array_equal(_bits(got[b]), _bits(want)), (case, b, g is not None)
    if case == "same_pixel":
        assert got.shape == (2, H, W) and _run_tracks(lib, tables, H, W, None)[0, 4, 5] == 2.0
    if case == "edges173":
        # the edge coordinates on their own: -1.0 lands on 0, -2.0 is outside, 2W - 0.5 lands on W - 1, 2W is outside, NaN and 1e300 are no pixel
        nan = float("nan")
        t = np.array([[0, -1.0, 2.0, 1.0], [1, -2.0, 2.0, 2.0], [2, 2 * W - 0.5, 2.0, 3.0], [3, 2.0 * W, 2.0, 4.0], [4, nan, 2.0, 5.0], [5, 1e300, 2.0, 6.0],
                      [6, 4.0, -1.0, 7.0], [7, 4.0, -2.0, 8.0], [8, 4.0, 2 * H - 0.5, 9.0], [9, 4.0, 2.0 * H, 10.0], [10, 4.0, nan, 11.0], [11, 4.0, 1e300, 12.0]])
        d = _run_tracks(lib, [t, np.zeros((0, 4))], H, W, None)
        assert (d[0, 1, 0], d[0, 1, W - 1], d[0, 0, 2], d[0, H - 1, 2]) == (1.0, 3.0, 7.0, 9.0) and np.count_nonzero(d) == 4


# ---- (c) vidc_nonzero_compact --------------------------------------------------------------------------------------------------------
def _nz_patterns(HW, ck):
    rng = np.random.RandomState(HW)
    pats = {"none": np.zeros(HW, np.float32), "all": rng.uniform(0.5, 5.0, HW).astype(np.float32)}
    first, last = np.zeros(HW, np.float32), np.zeros(HW, np.float32)
    first[0], last[-1] = 2.0, 3.0
    alt = np.zeros(HW, np.float32)
    alt[::2] = 1.5
    mixed = (rng.uniform(0.5, 5.0, HW) * (rng.uniform(size=HW) < 0.4)).astype(np.float32)
    mixed[rng.randint(0, HW)] = np.nan
    mixed[1 % HW] = -0.0
    mixed[(HW // 2)] = -0.0
    mixed[HW // 3] = np.nan
    mixed[HW - 1] = 1e-45                                           # the smallest denormal is not zero
    pats.update(first=first, last=last, alternating=alt, mixed=mixed)
    if HW > ck:
        full = np.zeros(HW, np.float32)
        full[:ck + 1] = 1.0                                         # a chunk with exactly chunk-size non-zeros, followed by one more
        late = np.zeros(HW, np.float32)
        c0 = (HW // ck - 1) * ck
        late[c0:min(c0 + ck + 1, HW)] = 1.0                         # ... the same in the last whole chunk
        pats.update(full_chunk=full, late_chunk=late)
    return pats


@gpu
@pytest.mark.parametrize("HW", [63, 256, 1961, 4160, 76800])
def test_hip_nonzero_compact(HW):
    lib, ck = _lib(), _L().NONZERO_CHUNK
    pats = _nz_patterns(HW, ck)
    names = list(pats)
    if HW == 76800:
        names = ["mixed", "full_chunk"]                             # the full-size map once
    B = 2
    for k, name in enumerate(names):
        v = np.stack([pats[name], pats[names[(k + 1) % len(names)]]])     # two different images per batch
        count, index = _Out((B,), torch.int32, -3), _Out((B, HW), torch.int32, -5)
        nb = lib.vidc_nonzero_compact_scratch_bytes(B, HW)
        assert nb == 4 * B * -(-HW // ck)
        sc = _scratch(nb)
        assert lib.vidc_nonzero_compact(_dev(v).data_ptr(), B, HW, count.ptr(), index.ptr(), sc.ptr(), _stream()) == 0
        sc.np()
        c, idx = count.np(), index.np()
        for b in range(B):
            want = np.flatnonzero(v[b])
            assert np.array_equal(want, torch.nonzero(torch.from_numpy(v[b])).reshape(-1).numpy())      # np.flatnonzero is torch.nonzero's order
            assert c[b] == len(want), (name, b)
            assert np.array_equal(idx[b, :c[b]], want), (name, b)
            assert np.all(idx[b, c[b]:] == -5), (name, b)           # the tail keeps its pre-fill
    nan_img = pats["mixed"]
    assert np.isnan(nan_img).any() and np.signbit(nan_img[nan_img == 0]).any()


# ---- (d) vidc_sparse_sample_scatter --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("HW", [63, 1961])
def test_hip_sparse_sample_scatter(HW):
    lib = _lib()
    rng = np.random.RandomState(HW)
    B = 4
    depth = (rng.uniform(0.5, 5.0, (B, HW)) * (rng.uniform(size=(B, HW)) < 0.6)).astype(np.float32)
    counts = [int(np.count_nonzero(depth[b])) for b in range(B)]
    index = np.full((B, HW), HW + 5, np.int32)                      # beyond count: values no kernel may use
    for b in range(B):
        index[b, :counts[b]] = np.flatnonzero(depth[b])
    want_n = [-1, 0, 1, counts[3] - 1]                              # a clone, and selections of 0, 1 and count - 1 in one batch
    perms = [np.zeros(0, np.int32)] + [rng.permutation(counts[b])[:want_n[b]].astype(np.int32) for b in range(1, B)]
    sel_off = np.cumsum([0] + [len(p) for p in perms])[:B].astype(np.int32)
    perm = np.concatenate(perms)
    out = _Out((B, HW), torch.float32, -7.0)
    assert lib.vidc_sparse_sample_scatter(_dev(depth).data_ptr(), _dev(index).data_ptr(), _dev(perm).data_ptr(), _dev(sel_off).data_ptr(),
                                          _dev(np.asarray(want_n, np.int32)).data_ptr(), max(want_n), B, HW, out.ptr(), _stream()) == 0
    got = out.np()
    for b in range(B):
        if want_n[b] < 0:
            want = depth[b]
        else:
            want = np.zeros(HW, np.float32)
            p = np.flatnonzero(depth[b])[perms[b]]
            want[p] = depth[b][p]
            assert np.count_nonzero(want) == want_n[b]
        assert np.array_equal(_bits(got[b]), _bits(want)), b
    # only clones: no selection table at all
    out = _Out((B, HW), torch.float32, -7.0)
    neg = _dev(np.full(B, -1, np.int32))
    assert lib.vidc_sparse_sample_scatter(_dev(depth).data_ptr(), _dev(index).data_ptr(), None, _dev(np.zeros(B, np.int32)).data_ptr(), neg.data_ptr(), 0, B, HW,
                                          out.ptr(), _stream()) == 0
    assert np.array_equal(_bits(out.np()), _bits(depth))


# ---- (e) vidc_resize_nearest_u16_depth_range -----------------------------------------------------------------------------------------
def _threshold_values(divisor, lo, hi):
    """16-bit values whose fp32 quotient lies below, exactly on (where one exists) and above fl(lo) and fl(hi)."""
    x = np.arange(65536, dtype=np.float32) / np.float32(divisor)
    vals = []
    for thr in (np.float32(lo), np.float32(hi)):
        k = int(np.searchsorted(x, thr))                            # first value with x >= thr
        vals += [k - 2, k - 1, k, k + 1]
    return [v for v in vals if 0 <= v < 65536]


@gpu
@pytest.mark.parametrize("sizes", SIZES)
def test_hip_nearest_depth_range(sizes):
    from vi_depth_completion_amd import preprocess
    lib = _lib()
    (h, w), (H, W) = sizes
    B = 2
    a = np.random.RandomState(13).randint(0, 65536, size=(B, h, w)).astype(np.uint16)
    a[0, ::3, ::5], a[1, 1, 1] = 0, 65535
    edge = _threshold_values(5000.0, 0.1, 7.0)
    assert 500 in edge and 35000 in edge                            # 500 / 5000 and 35000 / 5000 round to fl(0.1) and fl(7.0) themselves: kept
    assert np.float32(500) / np.float32(5000) == np.float32(0.1) and np.float32(35000) / np.float32(5000) == np.float32(7.0)
    a.reshape(B, -1)[:, :len(edge)] = edge                          # (a resize drops some of them: the identity-size call below holds them all)
    a.reshape(B, -1)[1, -len(edge):] = edge
    tx, ty = preprocess.nearest_table(w, W), preprocess.nearest_table(h, H)
    out = _Out((B, H, W), torch.float32, -7.0)
    x = _dev(a.view(np.int16))
    assert lib.vidc_resize_nearest_u16_depth_range(x.data_ptr(), out.ptr(), B, h, w, H, W, _dev(tx).data_ptr(), _dev(ty).data_ptr(), 5000.0, 0.1, 7.0,
                                                   _stream()) == 0
    got = out.np()
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(R.nyu_depth_literal(a[b], (W, H)).numpy()[0])), b
    # every threshold value, at identity size: below min -> 0, on min kept, on max kept, above max -> 0
    e = np.asarray(edge, np.uint16).reshape(1, 1, -1)
    n = e.shape[2]
    ident = _dev(np.arange(n, dtype=np.int32))
    out = _Out((1, 1, n), torch.float32, -7.0)
    assert lib.vidc_resize_nearest_u16_depth_range(_dev(e.view(np.int16)).data_ptr(), out.ptr(), 1, 1, n, 1, n, ident.data_ptr(), _dev(np.zeros(1, np.int32)).data_ptr(),
                                                   5000.0, 0.1, 7.0, _stream()) == 0
    got = out.np().reshape(-1)
    want = R.nyu_depth_literal(e[0], (n, 1)).numpy().reshape(-1)
    assert np.array_equal(_bits(got), _bits(want))
    d = dict(zip(edge, got))
    assert d[499] == 0 and d[500] == np.float32(0.1) and d[35000] == np.float32(7.0) and d[35001] == 0


@gpu
def test_hip_scannet_depth_is_the_existing_kernel_with_identity_tables():
    """dataset.py:124-126 through vidc_resize_nearest_u16_depth: all 65536 values."""
    from vi_depth_completion_amd.preprocess import ScanNetFramePreprocessor
    x = np.arange(65536, dtype=np.int64).astype(np.uint16).reshape(1, 256, 256)
    pre = ScanNetFramePreprocessor(DEV, hw=(256, 256))
    got = pre.gt_depth(_dev(x.view(np.int16)))
    assert _same(got[0], R.scannet_depth_literal(x[0]))


# ---- both classes end to end ---------------------------------------------------------------------------------------------------------
def _scannet_inputs(B, H, W, seed):
    rng = np.random.RandomState(seed)
    color = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    orient = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pred = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    mask = (rng.randint(0, 2, (B, H, W)) * 255).astype(np.uint8)
    mask[:, 0, :7] = [0, 1, 127, 128, 200, 254, 255]
    depth = rng.randint(300, 6000, (B, H, W)).astype(np.uint16)
    depth[rng.uniform(size=depth.shape) < 0.3] = 0
    gravity = np.array([[0.02, 0.97, 0.24], [0.1, 0.2, 0.97], [0.999, 0.0004, 0.0003]])[:B]      # up / gravity (cos <= 0.3) / psi < 1e-6
    tracks = [_tracks(n, H, W, seed + b) for b, n in zip(range(B), (173, 2500, 40))]
    return color, depth, orient, mask, gravity, tracks, pred


def _check_batch(got, want, shapes):
    assert set(got) == set(want) == set(shapes)
    for k in want:
        assert got[k].is_cuda and got[k].dtype == torch.float32 and tuple(got[k].shape) == shapes[k], (k, got[k].shape, got[k].dtype)
        assert _same(got[k].cpu(), want[k]), k


@gpu
@pytest.mark.parametrize("read_pointcloud", [True, False])
def test_hip_scannet_batch_equals_the_restatement(read_pointcloud):
    from vi_depth_completion_amd.preprocess import ScanNetFramePreprocessor
    B, H, W = 2, 240, 320
    color, depth, orient, mask, gravity, tracks, pred = _scannet_inputs(B, H, W, 21)
    want = R.collate([R.scannet_item(color[b], depth[b], orient[b], mask[b], gravity[b], tracks[b], pred[b], read_pointcloud=read_pointcloud) for b in range(B)])
    pre = ScanNetFramePreprocessor(DEV, read_depths_from_pointcloud=read_pointcloud)
    got = pre(color, depth, orient, mask, gravity, tracks, predicted_normal_u8=pred)
    shapes = {"image": (B, 3, H, W), "mask": (B, H, W), "depth": (B, 1, H, W), "gravity": (B, 3), "normal": (B, 3, H, W), "predicted_normal": (B, 3, H, W),
              "sparse_depth": (B, 1, H, W), "aligned_direction": (B, 3), "homogeneous_coordinates": (B, H, W, 3)}
    _check_batch(got, want, shapes)
    assert int((got["sparse_depth"] != 0).sum()) > 100
    # the same from tensors already on the device, without the optional key
    got2 = pre(_dev(color), _dev(depth.view(np.int16)), _dev(orient), _dev(mask), gravity, tracks)
    assert "predicted_normal" not in got2 and all(_same(got2[k].cpu(), want[k]) for k in got2)


@gpu
def test_hip_scannet_random_sparse_sample_follows_the_seeded_generator():
    from vi_depth_completion_amd.preprocess import ScanNetFramePreprocessor
    B, H, W = 3, 240, 320
    color, depth, orient, mask, gravity, tracks, _ = _scannet_inputs(B, H, W, 22)
    depth[1] = 0
    depth[1, 5, 6:40] = 1234                                        # 34 non-zero pixels against 2500 tracks: the clone
    tracks[2] = np.zeros((0, 4))                                    # a failed read: a permutation is drawn, nothing is kept
    ra, rb = np.random.RandomState(5), np.random.RandomState(5)
    want = R.collate([R.scannet_item(color[b], depth[b], orient[b], mask[b], gravity[b], tracks[b], random_sparse_pointcloud=True, rng=ra) for b in range(B)])
    pre = ScanNetFramePreprocessor(DEV, generate_random_sparse_pointcloud=True, rng=rb)
    got = pre(color, depth, orient, mask, gravity, tracks)
    shapes = {"image": (B, 3, H, W), "mask": (B, H, W), "depth": (B, 1, H, W), "gravity": (B, 3), "normal": (B, 3, H, W),
              "sparse_depth": (B, 1, H, W), "aligned_direction": (B, 3), "homogeneous_coordinates": (B, H, W, 3)}
    _check_batch(got, want, shapes)
    sd = got["sparse_depth"].cpu()
    assert [int((sd[b] != 0).sum()) for b in range(B)] == [173, 34, 0]
    sa, sb = ra.get_state(), rb.get_state()
    assert sa[2] == sb[2] and np.array_equal(sa[1], sb[1])
    assert ra.randint(0, 1 << 30) == rb.randint(0, 1 << 30)


@gpu
def test_hip_nyu_batch_equals_the_restatement():
    from vi_depth_completion_amd.preprocess import NYUFramePreprocessor
    B, H, W = 2, 240, 320
    rng = np.random.RandomState(31)
    color = rng.randint(0, 256, (B, 480, 640, 3)).astype(np.uint8)
    depth = rng.randint(0, 40000, (B, 480, 640)).astype(np.uint16)
    depth[:, 0, :8] = [0, 499, 500, 501, 34999, 35000, 35001, 65535]
    pred = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    tracks = [_tracks(173, H, W, 32, edge=True), np.zeros((0, 4))]
    want = R.collate([R.nyu_item(color[b], depth[b], tracks[b], pred[b]) for b in range(B)])
    pre = NYUFramePreprocessor(DEV)
    got = pre(color, depth, tracks, predicted_normal_u8=pred)
    _check_batch(got, want, {"image": (B, 3, H, W), "depth": (B, 1, H, W), "sparse_depth": (B, 1, H, W), "predicted_normal": (B, 3, H, W)})
    assert set(pre(color, depth, tracks)) == {"image", "depth", "sparse_depth"}


@gpu
def test_hip_classes_refuse_cpu_tensors_wrong_dtypes_and_shapes():
    from vi_depth_completion_amd.preprocess import NYUFramePreprocessor, ScanNetFramePreprocessor
    B, H, W = 1, 240, 320
    color, depth, orient, mask, gravity, tracks, pred = _scannet_inputs(B, H, W, 23)
    tracks = tracks[:B]
    pre = ScanNetFramePreprocessor(DEV)
    good = [_dev(color), _dev(depth.view(np.int16)), _dev(orient), _dev(mask), gravity, tracks]
    pre(*good)
    bad = [(0, torch.from_numpy(color)), (0, _dev(color).float()), (0, _dev(color)[:, :, :, :2]), (1, torch.from_numpy(depth.view(np.int16))),
           (1, _dev(depth.astype(np.int32))), (1, _dev(depth.view(np.int16))[:, :-1]), (2, _dev(orient)[:, 1:]), (3, _dev(mask).unsqueeze(-1)),
           (3, _dev(mask).to(torch.bool)), (4, np.zeros((B, 4)))]
    for i, v in bad:
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError):
            pre(*args)
    with pytest.raises(RuntimeError):
        pre(*good, predicted_normal_u8=torch.from_numpy(pred))
    nyu = NYUFramePreprocessor(DEV)
    c, d = np.zeros((1, 480, 640, 3), np.uint8), np.zeros((1, 480, 640), np.uint16)
    nyu(c, d, [np.zeros((0, 4))])
    for args in ((torch.from_numpy(c), d), (c[:, :240], d), (c, d.astype(np.float32)), (c, d[:, :, :320])):
        with pytest.raises(RuntimeError):
            nyu(*args, [np.zeros((0, 4))])
    with pytest.raises(RuntimeError):
        nyu(c, d, [np.zeros((0, 4))], predicted_normal_u8=np.zeros((1, 480, 640, 3), np.uint8))
