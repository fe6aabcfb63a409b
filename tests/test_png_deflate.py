"""The compressed PNG writer (csrc/png_deflate.hip, PngEncoder.encode_compressed, EvaluationWriter(compress=True)).  CPU: the restatement
tests/png_deflate_ref.py against Pillow's decoder and zlib's inflate, the size bound and the refusals of the C ABI.  GPU: every file parsed
field by field -- chunk CRCs, the fixed 1106-bit header, the inflated bytes equal to the restated filtered scanlines (filter choice, ties,
Adler), the symbol bits equal to the Huffman optimum, the size, Pillow's reading, the untouched bytes behind the largest file -- at the
shapes where the kernels take another path: one or several segments, a row longer than a segment, constant images, a histogram deeper
than 15 bits, batching, scratch reuse, and the --save writer."""
import os
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_deflate_ref as D  # noqa: E402
import png_ref as R  # noqa: E402
import test_png_writer as TW  # noqa: E402
from vi_depth_completion_amd import _lib as L  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402

gpu = pytest.mark.gpu
FORMATS, NAMES = TW.FORMATS, TW.NAMES
FILTERS = {D.FILTER_NONE: "none", D.FILTER_SUB: "sub", D.FILTER_UP: "up", D.FILTER_AVERAGE: "average", D.FILTER_PAETH: "paeth",
           D.FILTER_ADAPTIVE: "adaptive"}


def _smooth(fmt, B, H, W, seed):
    """B different images of ramps plus small noise (holes in the depth): the filters differ per row and the code lengths spread."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    k = np.arange(1, B + 1, dtype=np.float64).reshape(B, 1, 1)
    if fmt == R.DEPTH16_F32:
        d = 1.0 + 0.011 * x * k + 0.023 * y + rng.normal(0, 0.002, (B, H, W))
        d[:, :H // 3] = 1.0 + 3 * rng.uniform(size=(B, 1, W))                  # a band of columns that do not change down the rows
        d[rng.uniform(size=d.shape) < 0.05] = 0
        return np.maximum(d, 0)[:, None].astype(np.float32)
    if fmt == R.NORMAL8_F32:
        n = np.stack([0.4 * np.sin(x / 9.0 + k), 0.4 * np.cos(y / 7.0) + 0 * k, 1.0 + 0 * x + 0 * k], axis=1) + rng.normal(0, 0.004, (B, 3, H, W))
        return (n / np.sqrt((n * n).sum(1, keepdims=True))).astype(np.float32)
    if fmt == R.RGB8_F32:
        v = np.stack([x / W + 0 * k, y / H + 0 * k, (x + y * k) / (W + B * H)], axis=1) + rng.normal(0, 0.004, (B, 3, H, W))
        v[:, :, :H // 3] = rng.uniform(size=(B, 3, 1, W))
        return np.clip(v, 0, 1).astype(np.float32)
    m = ((3 * x + 5 * y * k) / 4 + rng.randint(0, 3, (B, H, W))).astype(np.int64).astype(np.uint8)
    m[:, :H // 3] = rng.randint(0, 256, (B, 1, W))
    return m


def _check_file(png, image, fmt, filt):
    """Everything a compressed file must be, against the restatement of ITS image; returns the parsed fields."""
    p = D.parse(png)                                                           # chunk order, every CRC, the file ends with IEND's CRC
    samp = R.samples(image, fmt)
    H, W = samp.shape[:2]
    stored = R.encode(image, fmt)
    assert p["ihdr"] == stored[16:29]
    assert p["payload"][:2] == b"\x78\x01" and p["prefix"] == D.header_prefix_bits()
    assert (p["bfinal"], p["btype"], p["hlit"], p["hdist"], p["hclen"]) == (1, 2, 0, 0, 15) and p["clc"] == [0, 0, 0] + [4] * 16
    want = D.filtered_scanlines(samp, filt)
    if p["data"] != want:
        got, ref = np.frombuffer(p["data"], np.uint8), np.frombuffer(want, np.uint8)
        assert len(got) == len(ref), (len(got), len(ref))
        bad = np.flatnonzero(got != ref)
        raise AssertionError("%d of %d filtered bytes differ, first at %d (row %d)" % (len(bad), len(ref), bad[0], bad[0] // (len(ref) // H)))
    hist, lengths = D.histogram(want), p["lengths"]
    assert lengths[257] == 0 and max(lengths) <= D.MAX_BITS and D.kraft(lengths[:257]) == 1 << D.MAX_BITS
    assert [b > 0 for b in lengths[:257]] == [c > 0 for c in hist]
    cost, depth = D.huffman_optimum(hist)
    print("%s %dx%d filter %d: %d bytes, symbol bits %d, optimum %d at depth %d" % (NAMES[fmt], H, W, filt, len(png), p["symbol_bits"], cost, depth))
    if depth <= D.MAX_BITS:
        assert p["symbol_bits"] == cost
    else:
        assert p["symbol_bits"] <= D.flat_bits(hist) * int(hist.sum())
    assert len(p["payload"]) == 2 + -(-(D.HEADER_BITS + p["symbol_bits"]) // 8) + 4
    bits = np.unpackbits(np.frombuffer(p["payload"][2:-4], np.uint8), bitorder="little")
    assert not bits[D.HEADER_BITS + p["symbol_bits"]:].any(), "pad bits"
    assert len(png) <= D.max_file_bytes(H, W, fmt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(TW._pillow_open(png), TW._pillow_open(stored))
    return p


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", sorted(FILTERS), ids=FILTERS.get)
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
@pytest.mark.parametrize("H,W", [(7, 5), (240, 320)])
def test_restatement_against_pillow_and_zlib(fmt, filt, H, W):
    img = (TW._images if filt % 2 else _smooth)(fmt, 1, H, W, 11 + fmt)[0]
    png = D.encode(img, fmt, filt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = TW._pillow_reference(img, fmt)
    got = TW._pillow_open(png)
    assert got.shape == want.shape and np.array_equal(got, want)
    samp = R.samples(img, fmt)
    assert zlib.decompress(R.idat_payload(png)) == D.filtered_scanlines(samp, filt)
    p = _check_file(png, img, fmt, filt)
    assert p["lengths"][:257] == list(D.package_merge(D.histogram(p["data"])))


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_smooth_images_choose_several_filters(fmt):
    """The smooth 33x41 images of the GPU cases do exercise the adaptive choice: at least three different filters per format."""
    f = D.row_filters(R.samples(_smooth(fmt, 3, 33, 41, 100 * fmt + 33)[0], fmt), D.FILTER_ADAPTIVE)
    assert len(set(f.tolist())) >= 3, f


def test_filters_against_the_specification_by_hand():
    """One 2x3 gray image worked out by hand (PNG specification 9.2-9.4), ties of the Paeth predictor included."""
    samp = np.array([[10, 20, 250], [30, 15, 5]], np.uint8)
    c = D.filter_candidates(samp)
    assert c[1].tolist() == [[10, 10, 230], [30, 241, 246]]
    assert c[2].tolist() == [[10, 20, 250], [20, 251, 11]]
    assert c[3].tolist() == [[10, 15, 240], [25, 246, 129]]                    # floor((a + b) / 2): (0+10)/2, (30+20)/2, (15+250)/2
    assert c[4].tolist() == [[10, 10, 230], [20, 241, 11]]                     # (30, 20, 10): p = 40, nearest is a = 30; (15, 250, 20): p = 245 -> b
    assert D.filtered_scanlines(samp, D.FILTER_ADAPTIVE)[0::4] == bytes(D.row_filters(samp, D.FILTER_ADAPTIVE))


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.lib()


def test_largest_file_through_the_c_abi(lib):
    for H, W, fmt in [(240, 320, R.DEPTH16_F32), (240, 320, R.NORMAL8_F32), (1, 1, R.GRAY8_U8), (3, 5, R.DEPTH16_F32), (7, 5, R.RGB8_F32),
                      (512, 512, R.GRAY8_U8)]:
        raw = H * (1 + W * R.LAYOUT[fmt][0])
        want = 57 + 2 + -(-(1106 + 9 * (raw + 1)) // 8) + 4
        assert lib.vidc_png_deflate_max_file_bytes(H, W, fmt) == want == D.max_file_bytes(H, W, fmt), (H, W, fmt)
        assert want <= 1.126 * lib.vidc_png_file_bytes(H, W, fmt) + 200
        assert lib.vidc_png_deflate_scratch_bytes(3, H, W, fmt) >= 3 * raw and lib.vidc_png_deflate_scratch_bytes(1, H, W, fmt) % 16 == 0
    assert lib.vidc_png_deflate_max_file_bytes(240, 320, R.DEPTH16_F32) == 57 + 2 + 173210 + 4 == 173273
    for H, W, fmt in [(0, 5, 0), (5, 0, 0), (-1, 5, 0), (5, 5, 4), (5, 5, -1), (40000, 40000, R.RGB8_F32)]:
        assert lib.vidc_png_deflate_max_file_bytes(H, W, fmt) == 0 and lib.vidc_png_deflate_scratch_bytes(1, H, W, fmt) == 0, (H, W, fmt)
    assert lib.vidc_png_deflate_scratch_bytes(0, 5, 5, 0) == 0


def test_encode_deflate_refuses_bad_arguments_without_gpu(lib):
    p, stride, A = 4096, 256, L.PNG_FILTER_ADAPTIVE                            # never dereferenced: every call below is refused first
    assert lib.vidc_png_deflate_max_file_bytes(3, 5, R.DEPTH16_F32) == 57 + 2 + 177 + 4 == 240 <= stride
    for args in [(None, 1, 3, 5, 0, A, p, stride, p, p), (p, 1, 3, 5, 0, A, None, stride, p, p), (p, 1, 3, 5, 0, A, p, stride, None, p),
                 (p, 1, 3, 5, 0, A, p, stride, p, None)]:
        assert lib.vidc_png_encode_deflate(*args, None) == -1 and b"null" in lib.vidc_last_error()
    for args in [(p, 0, 3, 5, 0, A, p, stride, p, p), (p, 1, 0, 5, 0, A, p, stride, p, p), (p, 1, 3, -2, 0, A, p, stride, p, p),
                 (p, 1, 3, 5, 4, A, p, stride, p, p),                          # unknown format
                 (p, 1, 3, 5, 0, 6, p, stride, p, p), (p, 1, 3, 5, 0, -1, p, stride, p, p),      # filter outside 0..5
                 (p, 1, 3, 5, 0, A, p, 112, p, p),                             # the stored file fits, the largest compressed one does not
                 (p, 1, 3, 5, 0, A, p, 248, p, p),                             # long enough, not a multiple of 16
                 (p, 1, 3, 5, 0, A, p + 4, stride, p, p),                      # files not 16-byte aligned
                 (p, 1, 40000, 40000, R.RGB8_F32, A, p, 1 << 40, p, p)]:       # beyond one IDAT chunk
        assert lib.vidc_png_encode_deflate(*args, None) == -2, args
    assert b"IDAT" in lib.vidc_last_error()


def _deep_mask():
    """512x512 mask whose byte values 1..19 have the counts 1, 1, 2, 4, ..., 2^17: with the 512 filter bytes 0 and the end-of-block the
    unrestricted Huffman code is 19 deep."""
    counts = [1] + [1 << k for k in range(18)]
    assert sum(counts) == 512 * 512
    vals = np.repeat(np.arange(1, 20, dtype=np.uint8), counts)
    np.random.RandomState(7).shuffle(vals)
    return vals.reshape(1, 512, 512)


def test_deep_histogram_is_deeper_than_15():
    hist = D.histogram(D.filtered_scanlines(_deep_mask()[0], D.FILTER_NONE))
    assert D.huffman_optimum(hist)[1] > D.MAX_BITS
    lengths = D.package_merge(hist)
    assert max(lengths) == 15 and D.kraft(lengths) == 1 << 15 and int((hist * lengths).sum()) <= D.flat_bits(hist) * int(hist.sum())


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _encode(enc, images, fmt, filt, extra=48):
    """The files of a batch through PngEncoder.encode_compressed into a buffer pre-filled with 0xA5, file_stride `extra` bytes over the
    minimum: from the largest file's size rounded up to 16 onward the bytes must still be 0xA5."""
    B, H, W = images.shape[0], images.shape[-2], images.shape[-1]
    n = (D.max_file_bytes(H, W, fmt) + 15) // 16 * 16
    out = torch.full((B, n + extra), 0xA5, dtype=torch.uint8, device="cuda")
    files, sizes = enc.encode_compressed(torch.from_numpy(images).cuda(), fmt, filt, out=out)
    assert files is out and sizes.dtype == torch.uint32 and tuple(sizes.shape) == (B,) and sizes.is_cuda
    host, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    assert (host[:, n:] == 0xA5).all(), "bytes behind the largest file were written"
    assert (sizes <= D.max_file_bytes(H, W, fmt)).all(), sizes
    return [host[i, :sizes[i]].tobytes() for i in range(B)]


def _encode_and_check(enc, images, fmt, filt, extra=48):
    got = _encode(enc, images, fmt, filt, extra)
    return got, [_check_file(png, images[i], fmt, filt) for i, png in enumerate(got)]


ADAPTIVE_SHAPES = [(f, H, W) for f in FORMATS for H, W in [(1, 1), (3, 5), (7, 5), (33, 41), (240, 320)]]


@gpu
@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("fmt,H,W", ADAPTIVE_SHAPES, ids=["%s-%dx%d" % (NAMES[f], H, W) for f, H, W in ADAPTIVE_SHAPES])
def test_adaptive_files(fmt, H, W, kind):
    from vi_depth_completion_amd.output import PngEncoder
    images = (TW._images if kind == "random" else _smooth)(fmt, 3, H, W, 100 * fmt + H)
    enc = PngEncoder()
    got, _ = _encode_and_check(enc, images, fmt, D.FILTER_ADAPTIVE)
    assert _encode(enc, images[1:2], fmt, D.FILTER_ADAPTIVE, extra=0)[0] == got[1]         # not on B, not on the stride


FIXED = [(f, H, W, k) for f in (R.DEPTH16_F32, R.RGB8_F32, R.GRAY8_U8) for H, W in [(7, 5), (33, 41)] for k in range(5)]


@gpu
@pytest.mark.parametrize("fmt,H,W,filt", FIXED, ids=["%s-%dx%d-%s" % (NAMES[f], H, W, FILTERS[k]) for f, H, W, k in FIXED])
def test_fixed_filters(fmt, H, W, filt):
    from vi_depth_completion_amd.output import PngEncoder
    _encode_and_check(PngEncoder(), _smooth(fmt, 2, H, W, 7 * fmt + filt), fmt, filt)


LONG = [(R.GRAY8_U8, 3, 5000), (R.RGB8_F32, 2, 1400), (R.DEPTH16_F32, 2, 2100),      # a row longer than one segment
        (R.GRAY8_U8, 4, 1023), (R.GRAY8_U8, 4, 1024)]                                # the raw size exactly at and just over a segment


@gpu
@pytest.mark.parametrize("fmt,H,W", LONG, ids=["%s-%dx%d" % (NAMES[f], H, W) for f, H, W in LONG])
def test_rows_and_segments_at_the_chunk_size(fmt, H, W):
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    _encode_and_check(enc, _smooth(fmt, 2, H, W, 3 * H + W), fmt, D.FILTER_ADAPTIVE)
    _encode_and_check(enc, TW._images(fmt, 1, H, W, H + W), fmt, D.FILTER_PAETH)


CONSTANT = [(R.DEPTH16_F32, 0.0), (R.DEPTH16_F32, 70.0), (R.NORMAL8_F32, 1.0), (R.NORMAL8_F32, -1.0), (R.GRAY8_U8, 0), (R.GRAY8_U8, 255)]


@gpu
@pytest.mark.parametrize("fmt,value", CONSTANT, ids=["%s-%s" % (NAMES[f], v) for f, v in CONSTANT])
def test_constant_images(fmt, value):
    """Under ADAPTIVE every filter of an all-zero image costs 0 and the tie goes to None: two used symbols.  An all-0xFF image costs
    |int8(0xFF)| per byte under None, one pixel under Sub (the first row) and nothing under Up.  Under NONE the mask 255 stream holds
    {0, 255, end-of-block} only."""
    from vi_depth_completion_amd.output import PngEncoder
    shape = (2, 240, 320) if fmt == R.GRAY8_U8 else (2, 1 if fmt == R.DEPTH16_F32 else 3, 240, 320)
    images = np.full(shape, value, np.uint8 if fmt == R.GRAY8_U8 else np.float32)
    enc = PngEncoder()
    _, parsed = _encode_and_check(enc, images, fmt, D.FILTER_ADAPTIVE)
    used = sum(b > 0 for b in parsed[0]["lengths"])
    if not np.any(R.samples(images[0], fmt)):
        assert set(parsed[0]["data"]) == {0} and used == 2                      # every row chose filter 0: the literal 0 and end-of-block
    else:
        assert used == 5, used                                                  # the first row under Sub, the others under Up: 1, 2, 0, 255 and end-of-block
    _, parsed = _encode_and_check(enc, images, fmt, D.FILTER_NONE)
    if fmt == R.GRAY8_U8 and value == 255:
        assert [s for s in range(257) if parsed[0]["lengths"][s]] == [0, 255, 256]


@gpu
def test_histogram_deeper_than_15_bits():
    from vi_depth_completion_amd.output import PngEncoder
    images = _deep_mask()
    hist = D.histogram(D.filtered_scanlines(images[0], D.FILTER_NONE))
    assert D.huffman_optimum(hist)[1] > D.MAX_BITS                              # before the GPU is touched
    _, parsed = _encode_and_check(PngEncoder(), images, R.GRAY8_U8, D.FILTER_NONE)
    best = int((hist * D.package_merge(hist)).sum())
    print("limited code %d bits, package-merge optimum %d, flat code %d" % (parsed[0]["symbol_bits"], best, D.flat_bits(hist) * int(hist.sum())))
    assert max(parsed[0]["lengths"]) <= D.MAX_BITS and best <= parsed[0]["symbol_bits"] <= D.flat_bits(hist) * int(hist.sum())


@gpu
def test_scratch_reuse():
    """Batch X, batch Y of the same shape, X again through one encoder with no synchronise in between: stale histograms, offsets or code
    tables in the shared scratch would change X's files."""
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    x, y = _smooth(R.DEPTH16_F32, 2, 60, 80, 5), TW._images(R.DEPTH16_F32, 2, 60, 80, 6)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    runs = [enc.encode_compressed(d, R.DEPTH16_F32) for d in (dx, dy, dx)]
    assert len(enc._scratch) == 1
    files = [[row[:n].tobytes() for row, n in zip(f.cpu().numpy(), s.cpu().numpy())] for f, s in runs]
    assert files[0] == files[2] and files[0] != files[1]
    for png, img in zip(files[0] + files[1], list(x) + list(y)):
        _check_file(png, img, R.DEPTH16_F32, D.FILTER_ADAPTIVE)
    enc.encode(dx, R.DEPTH16_F32)                                               # the stored scratch is another one
    assert len(enc._scratch) == 2


@gpu
def test_encode_compressed_refuses_what_encode_refuses():
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    with pytest.raises(RuntimeError):
        enc.encode_compressed(torch.zeros(1, 1, 4, 4), L.PNG_DEPTH16_F32)
    with pytest.raises(RuntimeError):
        enc.encode_compressed(torch.zeros(1, 4, 4, device="cuda"), L.PNG_GRAY8_U8)
    with pytest.raises(RuntimeError):
        enc.encode_compressed(torch.zeros(1, 2, 4, 4, device="cuda"), L.PNG_NORMAL8_F32)
    with pytest.raises(RuntimeError):
        enc.encode_compressed(torch.zeros(1, 1, 4, 4, device="cuda"), L.PNG_DEPTH16_F32, filter=6)
    with pytest.raises(RuntimeError):                                          # long enough for the stored file only
        enc.encode_compressed(torch.zeros(1, 1, 4, 4, device="cuda"), L.PNG_DEPTH16_F32, out=torch.zeros(1, 112, dtype=torch.uint8, device="cuda"))


@gpu
def test_evaluation_writer_compressed(tmp_path):
    """Five batches of two frames through two slots, both entry points, compress=True beside compress=False on the same tensors: the
    reference's names, every file a complete compressed file of ITS frame (so exactly sizes[i] bytes reached the disk) that Pillow reads
    as it reads the stored one."""
    from vi_depth_completion_amd import torch_ops  # noqa: F401
    from vi_depth_completion_amd.output import EvaluationWriter
    H, W, B, N = 60, 80, 2, 5
    pred = [_smooth(R.DEPTH16_F32, B, H, W, 200 + k) for k in range(N)]
    gt = [TW._images(R.DEPTH16_F32, B, H, W, 300 + k) for k in range(N)]
    npred = [_smooth(R.NORMAL8_F32, B, H, W, 400 + k) * np.float32(1.5) for k in range(N)]
    ngt = [TW._images(R.NORMAL8_F32, B, H, W, 500 + k) * np.float32(0.5) for k in range(N)]
    unit = lambda x: torch.ops.vidc.normalize_nchw(torch.from_numpy(x).cuda()).cpu().numpy()       # noqa: E731
    for name, compress in (("stored", False), ("packed", True)):
        with EvaluationWriter(str(tmp_path / name), slots=2, compress=compress) as wr:
            for k in range(N):
                batch = {"depth": torch.from_numpy(gt[k]), "normal": torch.from_numpy(ngt[k])}
                wr.save_evaluation_output(batch, torch.from_numpy(pred[k]).cuda(), k * B, pred_normals=torch.from_numpy(npred[k]).cuda())
            for k in range(N):
                names = ["color_%06d.png" % (1000 + 10 * (B * k + i)) for i in range(B)]
                wr.save_pred_only({"color_filename": names}, torch.from_numpy(pred[k]).cuda())
    stored, packed = tmp_path / "stored" / "evaluation_output", tmp_path / "packed" / "evaluation_output"
    want = sorted(["%s_%06d.png" % (p, j) for p in ("depth_pred", "depth_gt", "normal_pred", "normal_gt") for j in range(B * N)] +
                  ["depth_pred_%06d.png" % (1000 + 10 * j) for j in range(B * N)])
    assert sorted(os.listdir(packed)) == want == sorted(os.listdir(stored))
    for k in range(N):
        for prefix, data, fmt in (("depth_pred", pred[k], R.DEPTH16_F32), ("depth_gt", gt[k], R.DEPTH16_F32),
                                  ("normal_pred", unit(npred[k]), R.NORMAL8_F32), ("normal_gt", unit(ngt[k]), R.NORMAL8_F32)):
            for i in range(B):
                name = "%s_%06d.png" % (prefix, k * B + i)
                png = (packed / name).read_bytes()
                _check_file(png, data[i], fmt, D.FILTER_ADAPTIVE)
                assert (stored / name).read_bytes() == R.encode(data[i], fmt) and len(png) < len(R.encode(data[i], fmt)) * 1.13
        for i in range(B):
            _check_file((packed / ("depth_pred_%06d.png" % (1000 + 10 * (B * k + i)))).read_bytes(), pred[k][i], R.DEPTH16_F32, D.FILTER_ADAPTIVE)


@gpu
def test_demo_frame_compressed_is_smaller(seeded_weights, tmp_path):
    """Demo frame 000000 through the pipeline as test_png_writer.test_demo_frame_to_png_file sets it up, written stored and compressed: the
    same pixels, and the compressed depth and normal files are smaller (the CPU model gives 65 887 < 153 918 and 42 458 < 230 723)."""
    from PIL import Image
    from vi_depth_completion_amd.output import EvaluationWriter
    from vi_depth_completion_amd.pipeline import DepthCompletionPipeline, FixedPlaneMask
    from vi_depth_completion_amd.preprocess import FramePreprocessor
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    raw = np.load(os.path.join(golden, "preprocess_demo_000000.npz"))
    gold = np.load(os.path.join(golden, "demo_000000.npz"))
    pipe = DepthCompletionPipeline(enriched_samples=200)
    pipe.load_state_dicts(seeded_weights["sn"], seeded_weights["dc"])
    pipe.plane_masks_extraction = FixedPlaneMask(S.plane_id_map(240, 320))
    batch = FramePreprocessor("cuda")(raw["raw_rgb"][None], raw["gravity_raw"][None], [raw["klt_tracks"]])
    np.random.seed(int(gold["np_seed"]))
    taps = {}
    depth = pipe._call_cnn({k: v for k, v in batch.items()}, taps)
    normals = taps["normals"]
    assert tuple(normals.shape) == (1, 3, 240, 320)
    sample = {"depth": depth.cpu(), "normal": normals.cpu()}
    for name, compress in (("stored", False), ("packed", True)):
        with EvaluationWriter(str(tmp_path / name), compress=compress) as wr:
            wr.save_evaluation_output(sample, depth, 0, pred_normals=normals)
    want = np.minimum((depth.cpu().numpy()[0, 0] * 1000).astype(np.uint32), 65535)
    for png, stored_bytes in (("depth_pred_000000.png", 153918), ("normal_pred_000000.png", 230723)):
        a, b = (tmp_path / n / "evaluation_output" / png for n in ("stored", "packed"))
        pa, pb = np.asarray(Image.open(str(a))).astype(np.int64), np.asarray(Image.open(str(b))).astype(np.int64)
        assert np.array_equal(pa, pb) and (png[0] == "n" or np.array_equal(pb, want))
        print("%s: stored %d, compressed %d" % (png, os.path.getsize(a), os.path.getsize(b)))
        assert os.path.getsize(a) == stored_bytes and os.path.getsize(b) < stored_bytes
