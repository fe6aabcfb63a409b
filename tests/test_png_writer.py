"""The PNG writer (csrc/png.hip, vi_depth_completion_amd/output.py).  CPU: the restatement tests/png_ref.py against Pillow writing the
reference's own expressions (network_run.py:32-69), the file sizes and the refusals of the C ABI.  GPU: every file byte-equal to the
restatement -- every format at the shapes where the layout changes (odd widths, a block boundary at / before the end of the data and
inside a row, the workload's 3 and 4 blocks), the inputs on which the Adler sums would overflow, the values on which the conversions
round, batching, scratch reuse, and the --save writer with its ring of pinned buffers."""
import io
import os
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref as R  # noqa: E402
from vi_depth_completion_amd import _lib as L  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402

gpu = pytest.mark.gpu
FORMATS = (R.DEPTH16_F32, R.NORMAL8_F32, R.RGB8_F32, R.GRAY8_U8)
NAMES = {R.DEPTH16_F32: "depth16", R.NORMAL8_F32: "normal8", R.RGB8_F32: "rgb8", R.GRAY8_U8: "gray8"}
NORMAL_SWEEP = (np.arange(256) / 127.5 - 1).astype(np.float32)          # n = k / 127.5 - 1: where (1 + n) * 127.5 lands on the integers
DEPTH_EDGES = np.array([0, 1e-7, 0.0009999, 0.001, 65.5349, 65.535, 65.536, 70], np.float32)


def _images(fmt, B, H, W, seed):
    """B different images in the layout of the format's source tensor, inside the contract of the inputs."""
    rng = np.random.RandomState(seed)
    if fmt == R.DEPTH16_F32:
        d = rng.uniform(0, 12, (B, 1, H, W))
        d[rng.uniform(size=d.shape) < 0.1] = 0                                # holes
        far = rng.uniform(size=d.shape) < 0.05
        d[far] = rng.uniform(60, 70, int(far.sum()))                          # on both sides of the 65.535 m saturation
        return d.astype(np.float32)
    if fmt == R.NORMAL8_F32:
        n = rng.normal(size=(B, 3, H, W))
        return (n / np.sqrt((n * n).sum(1, keepdims=True))).astype(np.float32)
    if fmt == R.RGB8_F32:
        x = rng.uniform(0, 1, (B, 3, H, W))
        grid = rng.uniform(size=x.shape) < 0.3
        x[grid] = rng.randint(0, 256, int(grid.sum())) / 255.0                # the values a decoded 8-bit image holds
        return x.astype(np.float32)
    return rng.randint(0, 256, (B, H, W)).astype(np.uint8)


def _pillow_reference(img, fmt):
    """The array Pillow reads back from the file Pillow itself writes from the reference's expression."""
    from PIL import Image
    buf = io.BytesIO()
    if fmt == R.DEPTH16_F32:
        mm = (img.squeeze() * 1000).astype(np.uint32)                        # SaveDepthsToImage
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                               # Pillow 12: saving mode I as PNG is deprecated
                Image.fromarray(mm).save(buf, format="PNG")
        except (OSError, TypeError, ValueError):                              # a Pillow that refuses mode I: what it used to write, said directly
            buf = io.BytesIO()
            Image.fromarray(np.minimum(mm, 65535).astype(np.uint16)).save(buf, format="PNG")
    elif fmt == R.NORMAL8_F32:
        Image.fromarray(((1 + img.transpose([1, 2, 0])) * 127.5).astype(np.uint8)).save(buf, format="PNG")      # SaveNormalsToImage
    elif fmt == R.RGB8_F32:
        Image.fromarray(np.transpose(img * 255, axes=[1, 2, 0]).astype(np.uint8)).save(buf, format="PNG")      # SaveRgbToImage
    else:
        Image.fromarray(img).save(buf, format="PNG")                         # SaveMasksToImage
    return np.asarray(Image.open(io.BytesIO(buf.getvalue()))).astype(np.int64)


def _pillow_open(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png))).astype(np.int64)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
@pytest.mark.parametrize("H,W", [(7, 5), (240, 320)])
def test_restatement_against_pillow(fmt, H, W):
    img = _images(fmt, 1, H, W, 11 + fmt)[0]
    if fmt == R.DEPTH16_F32:
        img.reshape(-1)[:len(DEPTH_EDGES)] = DEPTH_EDGES
    png = R.encode(img, fmt)
    assert len(png) == R.file_bytes(H, W, fmt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = _pillow_reference(img, fmt)
    got = _pillow_open(png)
    assert got.shape == want.shape and np.array_equal(got, want)
    if fmt == R.DEPTH16_F32:
        assert got.max() == 65535 and np.array_equal(got, np.minimum((img[0] * 1000).astype(np.uint32), 65535))
    assert zlib.decompress(R.idat_payload(png)) == R.raw_scanlines(R.samples(img, fmt))


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.lib()


def test_file_sizes_through_the_c_abi(lib):
    for H, W, fmt, want in [(240, 320, R.DEPTH16_F32, 153918), (1, 1, R.DEPTH16_F32, 71), (3, 5, R.DEPTH16_F32, 101), (7, 5, R.RGB8_F32, 180),
                            (257, 254, R.GRAY8_U8, 65603), (258, 254, R.GRAY8_U8, 65863)]:
        assert lib.vidc_png_file_bytes(H, W, fmt) == want == R.file_bytes(H, W, fmt), (H, W, fmt)
        assert lib.vidc_png_scratch_bytes(3, H, W, fmt) == 3 * lib.vidc_png_scratch_bytes(1, H, W, fmt) > 0
    for H, W, fmt in [(0, 5, 0), (5, 0, 0), (-1, 5, 0), (5, 5, 4), (5, 5, -1), (40000, 40000, R.RGB8_F32)]:
        assert lib.vidc_png_file_bytes(H, W, fmt) == 0 and lib.vidc_png_scratch_bytes(1, H, W, fmt) == 0, (H, W, fmt)
    assert lib.vidc_png_scratch_bytes(0, 5, 5, 0) == 0


def test_encode_refuses_bad_arguments_without_gpu(lib):
    p, stride = 4096, 160                                                      # never dereferenced: every call below is refused first
    assert lib.vidc_png_file_bytes(3, 5, R.DEPTH16_F32) == 101
    for args in [(None, 1, 3, 5, 0, p, stride, p), (p, 1, 3, 5, 0, None, stride, p), (p, 1, 3, 5, 0, p, stride, None)]:
        assert lib.vidc_png_encode(*args, None) == -1 and b"null" in lib.vidc_last_error()
    for args in [(p, 0, 3, 5, 0, p, stride, p), (p, 1, 0, 5, 0, p, stride, p), (p, 1, 3, -2, 0, p, stride, p), (p, 1, 3, 5, 4, p, stride, p),
                 (p, 1, 3, 5, 0, p, 96, p),               # shorter than the file
                 (p, 1, 3, 5, 0, p, 104, p),              # long enough, not a multiple of 16
                 (p, 1, 3, 5, 0, p + 4, stride, p),       # files not 16-byte aligned
                 (p, 1, 40000, 40000, R.RGB8_F32, p, 1 << 40, p)]:      # beyond one IDAT chunk
        assert lib.vidc_png_encode(*args, None) == -2, args
    assert b"IDAT" in lib.vidc_last_error()


def test_normal_sweep_tells_the_two_roundings_apart():
    """(1 + n) * 127.5 in two rounded operations is what numpy computes; a fused multiply-add gives another byte for some n = k / 127.5 - 1,
    so the sweep of the GPU test below does tell a kernel that contracts the expression from one that does not."""
    n = np.broadcast_to(NORMAL_SWEEP, (3, 1, 256))
    assert (R.normal_samples(n) != R.normal_samples_fused(n)).any()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _encode(enc, images, fmt, extra=48):
    """The files of a batch through PngEncoder into a buffer pre-filled with 0xA5, file_stride `extra` bytes over the minimum: the padding
    must still be 0xA5 afterwards."""
    B, H, W = images.shape[0], images.shape[-2], images.shape[-1]
    n = R.file_bytes(H, W, fmt)
    out = torch.full((B, (n + 15) // 16 * 16 + extra), 0xA5, dtype=torch.uint8, device="cuda")
    files, nb = enc.encode(torch.from_numpy(images).cuda(), fmt, out=out)
    assert nb == n and files is out
    host = out.cpu().numpy()
    assert (host[:, n:] == 0xA5).all(), "bytes behind the file were written"
    return [host[i, :n].tobytes() for i in range(B)]


def _assert_files(got, images, fmt):
    for i, png in enumerate(got):
        want = R.encode(images[i], fmt)
        if png != want:
            bad = np.flatnonzero(np.frombuffer(png, np.uint8) != np.frombuffer(want, np.uint8))
            raise AssertionError("image %d: %d of %d bytes differ, first at offset %d" % (i, len(bad), len(want), bad[0]))


SHAPES = ([(f, H, W) for f in FORMATS for H, W in [(1, 1), (3, 5), (7, 5), (240, 320), (256, 320)]] +
          [(R.GRAY8_U8, 257, 254), (R.GRAY8_U8, 258, 254), (R.RGB8_F32, 69, 316), (R.RGB8_F32, 70, 316)])


@gpu
@pytest.mark.parametrize("fmt,H,W", SHAPES, ids=["%s-%dx%d" % (NAMES[f], H, W) for f, H, W in SHAPES])
def test_files_equal_the_restatement(fmt, H, W):
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    images = _images(fmt, 3, H, W, 100 * fmt + H)
    got = _encode(enc, images, fmt)
    _assert_files(got, images, fmt)
    assert _encode(enc, images[1:2], fmt, extra=0)[0] == got[1]               # an image's bytes do not depend on B or on the stride
    if (H, W) == (240, 320):
        for i, png in enumerate(got):                                          # ... and Pillow reads the reference expression's values back
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(_pillow_open(png), _pillow_reference(images[i], fmt))


@gpu
@pytest.mark.parametrize("fmt,value", [(R.DEPTH16_F32, 70.0), (R.RGB8_F32, 1.0), (R.NORMAL8_F32, 1.0), (R.DEPTH16_F32, 0.0), (R.RGB8_F32, 0.0),
                                       (R.NORMAL8_F32, -1.0)])
def test_constant_images(fmt, value):
    """All-0xFF samples at 240x320 (depth 70 m, rgb / normal 1.0): the input on which the Adler sums overflow without the modulus; all-zero
    samples are the companion."""
    from vi_depth_completion_amd.output import PngEncoder
    images = np.full((2, 1 if fmt == R.DEPTH16_F32 else 3, 240, 320), value, np.float32)
    assert set(np.unique(R.samples(images[0], fmt))) <= {0, 255, 65535}
    _assert_files(_encode(PngEncoder(), images, fmt), images, fmt)


@gpu
def test_constant_masks():
    from vi_depth_completion_amd.output import PngEncoder
    for v in (255, 0):
        images = np.full((2, 240, 320), v, np.uint8)
        _assert_files(_encode(PngEncoder(), images, R.GRAY8_U8), images, R.GRAY8_U8)


@gpu
def test_values_where_the_conversions_round():
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    depth = np.resize(DEPTH_EDGES, (1, 1, 3, 8)).astype(np.float32)
    assert set(R.depth_samples(depth[0, 0]).reshape(-1)) >= {0, 1, 65534, 65535}
    _assert_files(_encode(enc, depth, R.DEPTH16_F32), depth, R.DEPTH16_F32)
    sweep = np.concatenate([NORMAL_SWEEP, np.float32([1, -1])])
    normals = np.stack([np.roll(sweep, 7 * c) for c in range(3)]).reshape(1, 3, 2, 129)
    assert (R.normal_samples(normals[0]) != R.normal_samples_fused(normals[0])).any()
    _assert_files(_encode(enc, normals, R.NORMAL8_F32), normals, R.NORMAL8_F32)
    grid = (np.arange(256) / 255.0).astype(np.float32)
    rgb = np.stack([np.roll(grid, 11 * c) for c in range(3)]).reshape(1, 3, 4, 64)
    assert set(R.rgb_samples(rgb[0]).reshape(-1)) == set(range(256))
    _assert_files(_encode(enc, rgb, R.RGB8_F32), rgb, R.RGB8_F32)


@gpu
def test_back_to_back_encodes_share_the_scratch():
    """Two batches of one shape through one PngEncoder on one stream with no synchronise between them: the second call reuses the first
    one's scratch buffer, and stream order keeps the two apart."""
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    a, b = _images(R.DEPTH16_F32, 2, 240, 320, 5), _images(R.DEPTH16_F32, 2, 240, 320, 6)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    fa, n = enc.encode_depth(da)
    fb, _ = enc.encode_depth(db)
    assert len(enc._scratch) == 1 and fa.shape[1] % 16 == 0 and fa.shape[1] - n < 16
    _assert_files([r[:n].tobytes() for r in fa.cpu().numpy()], a, R.DEPTH16_F32)
    _assert_files([r[:n].tobytes() for r in fb.cpu().numpy()], b, R.DEPTH16_F32)


@gpu
def test_encoder_refuses_cpu_tensors_and_wrong_dtypes():
    from vi_depth_completion_amd.output import PngEncoder
    enc = PngEncoder()
    with pytest.raises(RuntimeError):
        enc.encode_depth(torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError):
        enc.encode_depth(torch.zeros(1, 1, 4, 4, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        enc.encode_mask(torch.zeros(1, 4, 4, device="cuda"))
    with pytest.raises(RuntimeError):
        enc.encode_normals(torch.zeros(1, 2, 4, 4, device="cuda"))


@gpu
def test_evaluation_writer_ring(tmp_path):
    """Seven batches of two frames through two slots with no flush in between, both entry points: the names the reference builds, and every
    file the restatement of ITS OWN frame -- a slot that is overwritten before its files are on disk shows here."""
    from vi_depth_completion_amd import torch_ops  # noqa: F401
    from vi_depth_completion_amd.output import EvaluationWriter
    H, W, B, N = 60, 80, 2, 7
    pred = [_images(R.DEPTH16_F32, B, H, W, 200 + k) for k in range(N)]
    gt = [_images(R.DEPTH16_F32, B, H, W, 300 + k) for k in range(N)]
    npred = [_images(R.NORMAL8_F32, B, H, W, 400 + k) * np.float32(1.5) for k in range(N)]          # not unit length: the writer normalises
    ngt = [_images(R.NORMAL8_F32, B, H, W, 500 + k) * np.float32(0.5) for k in range(N)]
    unit = lambda x: torch.ops.vidc.normalize_nchw(torch.from_numpy(x).cuda()).cpu().numpy()       # noqa: E731
    with EvaluationWriter(str(tmp_path / "demo"), slots=2) as wr:
        for k in range(N):
            names = ["color_%06d.png" % (1000 + 10 * (B * k + i)) for i in range(B)]
            wr.save_pred_only({"color_filename": names}, torch.from_numpy(pred[k]).cuda())
        wr.flush()
        out = tmp_path / "demo" / "evaluation_output"
        assert sorted(os.listdir(out)) == ["depth_pred_%06d.png" % (1000 + 10 * j) for j in range(B * N)]
        for k in range(N):
            _assert_files([(out / ("depth_pred_%06d.png" % (1000 + 10 * (B * k + i)))).read_bytes() for i in range(B)], pred[k], R.DEPTH16_F32)
    with EvaluationWriter(str(tmp_path / "eval"), slots=2) as wr:
        for k in range(N):
            batch = {"depth": torch.from_numpy(gt[k]), "normal": torch.from_numpy(ngt[k])}
            wr.save_evaluation_output(batch, torch.from_numpy(pred[k]).cuda(), k * B, pred_normals=torch.from_numpy(npred[k]).cuda())
        wr.save_evaluation_output({"depth": torch.from_numpy(gt[0])}, torch.from_numpy(pred[0]).cuda(), N * B)      # a depth-only network
    out = tmp_path / "eval" / "evaluation_output"
    assert sorted(os.listdir(out)) == sorted(["%s_%06d.png" % (p, j) for p in ("depth_pred", "depth_gt") for j in range(B * N + B)] +
                                             ["%s_%06d.png" % (p, j) for p in ("normal_pred", "normal_gt") for j in range(B * N)])
    for k in range(N):
        for prefix, data, fmt in (("depth_pred", pred[k], R.DEPTH16_F32), ("depth_gt", gt[k], R.DEPTH16_F32),
                                  ("normal_pred", unit(npred[k]), R.NORMAL8_F32), ("normal_gt", unit(ngt[k]), R.NORMAL8_F32)):
            _assert_files([(out / ("%s_%06d.png" % (prefix, k * B + i))).read_bytes() for i in range(B)], data, fmt)
    _assert_files([(out / ("depth_pred_%06d.png" % (N * B + i))).read_bytes() for i in range(B)], pred[0], R.DEPTH16_F32)


@gpu
def test_demo_frame_to_png_file(seeded_weights, tmp_path):
    """Demo frame 000000 from the raw 640x480 RGB + gravity + KLT tracks to the file the demo leaves behind (demo.sh: main.py --save):
    FramePreprocessor -> _call_cnn -> save_pred_only, and Pillow reads depth_pred_000000.png back as the reference's millimetres."""
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
    depth = pipe._call_cnn({k: v for k, v in batch.items()})
    with EvaluationWriter(str(tmp_path)) as wr:
        wr.save_pred_only({"color_filename": ["color_000000.png"]}, depth)
    got = np.asarray(Image.open(str(tmp_path / "evaluation_output" / "depth_pred_000000.png")))
    want = np.minimum((depth.cpu().numpy()[0, 0] * 1000).astype(np.uint32), 65535)
    assert got.shape == (240, 320) and np.array_equal(got.astype(np.int64), want) and 0 < want.max() < 20000
