#!/usr/bin/env python3
"""Times the PNG writer (csrc/png.hip, vi_depth_completion_amd/output.py) on the GPU against the reference's host writer.

For 240x320 and 256x320, B = 1, 4, 8 and each of the four formats:
  * the encode alone (two launches): device events around a run of calls, and a host clock around the same run ending in a synchronise;
  * files/s of encode + copy + write into a temporary directory through EvaluationWriter's ring, and of the same frames written the
    reference's way (`.cpu().numpy()`, the Save*ToImage expression, Pillow, one thread) in the same process, alternating, each leg at
    least --seconds long, --repeats times for the spread.
One more leg runs the frame stream `run_interleaved(lanes=3, frames_per_launch=4)` with the writer attached against the same stream
without it.  Nothing here has a pass mark; a leg that cannot run is reported as "not measured" with the reason.

    python tools/png_writer_bench.py [--seconds 1.0] [--repeats 3] [--out profiles/png_writer.json] [--no-stream-leg]

--compress measures the compressed writer (csrc/png_deflate.hip) instead, into profiles/png_deflate.json: at 240x320, B = 1, 8, 32 and each
format, files/s of encode_compressed against encode (alternating, device events) and against Pillow on this host; the file sizes on the
golden demo frame against the stored files and Pillow's; the cost of the 15-bit-limited code on an over-deep histogram against the
package-merge optimum; and the frame stream with EvaluationWriter(compress=True) against compress=False and against no writer.

    python tools/png_writer_bench.py --compress [--seconds 1.0] [--repeats 3] [--out profiles/png_deflate.json] [--no-stream-leg]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vi_depth_completion_amd import _lib as L                             # noqa: E402
from vi_depth_completion_amd import synthetic as S                        # noqa: E402
from vi_depth_completion_amd.output import EvaluationWriter, PngEncoder   # noqa: E402

FORMATS = ((L.PNG_DEPTH16_F32, "depth16"), (L.PNG_NORMAL8_F32, "normal8"), (L.PNG_RGB8_F32, "rgb8"), (L.PNG_GRAY8_U8, "gray8"))


def make_source(fmt, B, H, W):
    g = torch.Generator().manual_seed(1000 * fmt + B + H)
    if fmt == L.PNG_DEPTH16_F32:
        x = torch.rand((B, 1, H, W), generator=g) * 8 + 0.3              # a smooth-ish indoor range would compress better; Pillow's time depends on it little
    elif fmt == L.PNG_NORMAL8_F32:
        x = torch.nn.functional.normalize(torch.randn((B, 3, H, W), generator=g), dim=1)
    elif fmt == L.PNG_RGB8_F32:
        x = torch.rand((B, 3, H, W), generator=g)
    else:
        x = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    return x.cuda()


def time_encode(enc, src, fmt, seconds, compressed=False):
    """(microseconds per call by device events, by the host clock around the same calls + synchronise, calls timed)"""
    encode = enc.encode_compressed if compressed else enc.encode
    for _ in range(10):
        encode(src, fmt)
    torch.cuda.synchronize()
    ev_ms = host_s = 0.0
    calls, chunk = 0, 100
    while host_s < seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(chunk):
            encode(src, fmt)
        e1.record()
        torch.cuda.synchronize()
        host_s += time.perf_counter() - t0
        ev_ms += e0.elapsed_time(e1)
        calls += chunk
    return ev_ms * 1e3 / calls, host_s * 1e6 / calls, calls


def device_files_per_s(writer, src, fmt, seconds):
    B = src.shape[0]
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        writer._submit([("bench_", src, fmt)], list(range(B)))
        n += B
    writer.flush()
    return n / (time.perf_counter() - t0)


def pillow_save(arr, fmt, path):
    """The body of SaveDepthsToImage / SaveNormalsToImage / SaveRgbToImage / SaveMasksToImage (network_run.py:32-69)."""
    from PIL import Image
    if fmt == L.PNG_DEPTH16_F32:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # Pillow 12: saving mode I as PNG is deprecated
            Image.fromarray((arr.squeeze() * 1000).astype(np.uint32)).save(path)
    elif fmt == L.PNG_NORMAL8_F32:
        Image.fromarray(((1 + arr.transpose([1, 2, 0])) * 127.5).astype(np.uint8)).save(path)
    elif fmt == L.PNG_RGB8_F32:
        Image.fromarray(np.transpose(arr * 255, axes=[1, 2, 0]).astype(np.uint8)).save(path)
    else:
        Image.fromarray(arr).save(path)


def pillow_files_per_s(src, fmt, out_dir, seconds):
    B = src.shape[0]
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for i in range(B):
            pillow_save(src[i].detach().cpu().numpy(), fmt, os.path.join(out_dir, "pillow_%06d.png" % i))
        n += B
    return n / (time.perf_counter() - t0)


def spread(v):
    return {"runs": [round(x, 1) for x in v], "median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def stream_leg(out_dir, frames, repeats, compress=False):
    """frames/s of the stream mode bench.py times (256x320, batch 1, lanes 3, four items per launch) with save_pred_only on every output,
    against the same loop without it; alternating."""
    H, W, dev = 256, 320, torch.device("cuda:0")
    from vi_depth_completion_amd.pipeline import DepthCompletionPipeline, FixedPlaneMask
    cc = (0.5 * 319.87654 * W / 320.0, 0.5 * 239.87603 * H / 240.0)
    pipe = DepthCompletionPipeline(enriched_samples=200, cc_img=cc, device=dev, rng=np.random.RandomState(1234))
    pipe.load_state_dicts(S.seeded_state_dict(pipe.surface_normal_cnn.state_dict(), 1234, device=dev),
                          S.seeded_state_dict(pipe.cnn.state_dict(), 1234, device=dev))
    pipe.plane_masks_extraction = FixedPlaneMask(S.plane_id_map(H, W))
    pool = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in S.synthetic_batch(1, H, W, 1234, frame0=j).items()} for j in range(4)]

    def run(n, writer):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, out in enumerate(pipe.run_interleaved((pool[j % 4] for j in range(n)), lanes=3, frames_per_launch=4)):
            if writer is not None:
                writer.save_pred_only({"color_filename": ["color_%06d.png" % i]}, out)
        if writer is not None:
            writer.flush()
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    pipe.prepare_interleaved(pool[0], lanes=3, frames_per_launch=4)
    res = {"height": H, "width": W, "lanes": 3, "frames_per_launch": 4, "frames_per_run": frames}
    with EvaluationWriter(out_dir, slots=4) as writer, EvaluationWriter(out_dir + "_compressed", slots=4, compress=compress) as packed:
        legs = [("without_writer", None), ("with_writer", writer)] + ([("with_compressing_writer", packed)] if compress else [])
        for _, w in legs:
            run(48, w)
        rates = {name: [] for name, _ in legs}
        for _ in range(repeats):
            for name, w in legs:
                rates[name].append(run(frames, w))
    res.update({"frames_per_s_" + name: spread(v) for name, v in rates.items()})
    return res


def smooth_source(fmt, B, H, W):
    """Ramps plus a little noise, holes in the depth: the statistics of a prediction rather than of noise (make_source), so that the
    histograms, the code lengths and the file sizes are those of the workload."""
    g = torch.Generator().manual_seed(2000 * fmt + B + H)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    k = torch.arange(1, B + 1, dtype=torch.float32).reshape(B, 1, 1, 1)
    if fmt == L.PNG_DEPTH16_F32:
        v = 1.0 + 0.004 * x + 0.006 * y * (1 + 0.1 * k) + 0.002 * torch.randn((B, 1, H, W), generator=g)
        v[torch.rand((B, 1, H, W), generator=g) < 0.02] = 0
    elif fmt == L.PNG_NORMAL8_F32:
        v = torch.stack([0.4 * torch.sin(x / 40), 0.4 * torch.cos(y / 30), torch.ones_like(x)]).unsqueeze(0) + 0.02 * k + 0.004 * torch.randn((B, 3, H, W), generator=g)
        v = torch.nn.functional.normalize(v, dim=1)
    elif fmt == L.PNG_RGB8_F32:
        v = (torch.stack([x / W, y / H, (x + y) / (W + H)]).unsqueeze(0) * (1 - 0.01 * k) + 0.004 * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)
    else:
        v = (((x / 40).floor() + (y / 30).floor() * k.reshape(B, 1, 1)) % 7).to(torch.uint8)          # a plane-id map
    return v.contiguous().cuda()


def pillow_bytes(arr, fmt, tmp):
    path = os.path.join(tmp, "size.png")
    pillow_save(arr, fmt, path)
    return os.path.getsize(path)


def compress_main(a):
    """The compressed writer: profiles/png_deflate.json."""
    import PIL
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import png_deflate_ref as D
    H, W = 240, 320
    res = {"device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "seconds_per_leg": a.seconds, "repeats": a.repeats, "H": H, "W": W,
           "encode": [], "sizes": []}
    enc = PngEncoder()
    with tempfile.TemporaryDirectory(prefix="vidc_png_bench_") as tmp:
        for B in (1, 8, 32):
            for fmt, name in FORMATS:
                src = smooth_source(fmt, B, H, W)
                stored, packed = [], []
                for _ in range(a.repeats):                                  # alternating: the two encoders of one build under one load
                    stored.append(B * 1e6 / time_encode(enc, src, fmt, a.seconds / 4)[0])
                    packed.append(B * 1e6 / time_encode(enc, src, fmt, a.seconds / 4, compressed=True)[0])
                try:
                    ref = spread([pillow_files_per_s(src, fmt, tmp, a.seconds / 2) for _ in range(a.repeats)])
                except (OSError, TypeError, ValueError) as e:
                    ref = "not measured: Pillow %s refuses (%s)" % (PIL.__version__, e)
                sizes = enc.encode_compressed(src, fmt)[1].cpu().numpy()
                row = {"B": B, "format": name, "stored_file_bytes": enc.file_bytes(H, W, fmt), "compressed_file_bytes_mean": round(float(sizes.mean()), 1),
                       "encode_files_per_s": spread(stored), "encode_compressed_files_per_s": spread(packed), "pillow_files_per_s_incl_copy": ref}
                res["encode"].append(row)
                print(json.dumps(row), flush=True)
        # ---- the golden demo frames (tests/golden/demo_0000??.npz: the reference's outputs under the seeded weights) and a plane-id map
        names = ["demo_%06d" % i for i in range(0, 120, 17)]
        gold = [np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")) for n in names]
        frames = [(L.PNG_DEPTH16_F32, "depth16", np.stack([g["depth"][None] for g in gold]).astype(np.float32)),
                  (L.PNG_NORMAL8_F32, "normal8", np.stack([g["normals"] for g in gold]).astype(np.float32)),
                  (L.PNG_RGB8_F32, "rgb8", np.stack([g["image_u8"].transpose(2, 0, 1) / 255.0 for g in gold]).astype(np.float32)),
                  (L.PNG_GRAY8_U8, "gray8", S.plane_id_map(H, W).astype(np.uint8)[None])]
        for fmt, name, arr in frames:
            row = {"images": names if fmt != L.PNG_GRAY8_U8 else ["plane_id_map"], "format": name, "stored": enc.file_bytes(H, W, fmt)}
            for filt, fname in ((L.PNG_FILTER_ADAPTIVE, "adaptive"), (L.PNG_FILTER_NONE, "none"), (L.PNG_FILTER_SUB, "sub"), (L.PNG_FILTER_UP, "up"),
                                (L.PNG_FILTER_AVERAGE, "average"), (L.PNG_FILTER_PAETH, "paeth")):
                sizes = enc.encode_compressed(torch.from_numpy(arr).cuda(), fmt, filt)[1].cpu().numpy()
                row["compressed_%s_mean" % fname] = round(float(sizes.mean()), 1)
                if filt == L.PNG_FILTER_ADAPTIVE:
                    row["compressed_adaptive_each"] = [int(v) for v in sizes]
            try:
                each = [pillow_bytes(x, fmt, tmp) for x in arr]
                row["pillow_mean"], row["pillow_each"] = round(float(np.mean(each)), 1), each
            except (OSError, TypeError, ValueError) as e:
                row["pillow_mean"] = "not measured: Pillow %s refuses (%s)" % (PIL.__version__, e)
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
        # ---- the 15-bit limit: byte values 1..19 with the counts 1, 1, 2, 4, ..., 2^17 in a 512x512 mask under filter None
        vals = np.repeat(np.arange(1, 20, dtype=np.uint8), [1] + [1 << k for k in range(18)])
        np.random.RandomState(7).shuffle(vals)
        files, sizes = enc.encode_compressed(torch.from_numpy(vals.reshape(1, 512, 512)).cuda(), L.PNG_GRAY8_U8, L.PNG_FILTER_NONE)
        p = D.parse(files[0, :int(sizes[0])].cpu().numpy().tobytes())
        hist = D.histogram(p["data"])
        best = int((hist * D.package_merge(hist)).sum())
        res["over_deep"] = {"unrestricted_depth": D.huffman_optimum(hist)[1], "unrestricted_bits": D.huffman_optimum(hist)[0], "limited_bits": p["symbol_bits"],
                            "package_merge_bits": best, "excess_bits": p["symbol_bits"] - best, "flat_code_bits": D.flat_bits(hist) * int(hist.sum())}
        print(json.dumps(res["over_deep"]), flush=True)
        if a.no_stream_leg:
            res["stream"] = "not measured: --no-stream-leg"
        else:
            res["stream"] = stream_leg(os.path.join(tmp, "stream"), a.stream_frames, a.repeats, compress=True)
            print("stream:", json.dumps(res["stream"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="least length of a files/s leg (the encode-only legs take a quarter of it)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--compress", action="store_true", help="measure the compressed writer instead (profiles/png_deflate.json)")
    ap.add_argument("--out", default=None, help="default: profiles/png_writer.json, with --compress profiles/png_deflate.json")
    ap.add_argument("--no-stream-leg", action="store_true")
    ap.add_argument("--stream-frames", type=int, default=600)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_writer_bench needs a GPU: a timing taken without one says nothing")
    import PIL
    torch.set_grad_enabled(False)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "png_deflate.json" if a.compress else "png_writer.json")
    if a.compress:
        return compress_main(a)
    res = {"device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "seconds_per_leg": a.seconds, "repeats": a.repeats, "encode": [], "write": []}
    enc = PngEncoder()
    with tempfile.TemporaryDirectory(prefix="vidc_png_bench_") as tmp:
        with EvaluationWriter(tmp, slots=4) as writer:
            for H, W in ((240, 320), (256, 320)):
                for B in (1, 4, 8):
                    for fmt, name in FORMATS:
                        src = make_source(fmt, B, H, W)
                        ev_us, host_us, calls = time_encode(enc, src, fmt, a.seconds / 4)
                        nbytes = enc.file_bytes(H, W, fmt)
                        res["encode"].append({"H": H, "W": W, "B": B, "format": name, "file_bytes": nbytes, "calls": calls,
                                              "us_per_call_device_events": round(ev_us, 2), "us_per_call_host_clock": round(host_us, 2)})
                        row = {"H": H, "W": W, "B": B, "format": name}
                        ours, ref, why = [], [], None
                        for _ in range(a.repeats):
                            ours.append(device_files_per_s(writer, src, fmt, a.seconds))
                            if why is None:
                                try:
                                    ref.append(pillow_files_per_s(src, fmt, tmp, a.seconds))
                                except (OSError, TypeError, ValueError) as e:          # e.g. a Pillow that no longer writes mode I
                                    why = "not measured: Pillow %s refuses (%s)" % (PIL.__version__, e)
                        row["device_files_per_s"] = spread(ours)
                        row["pillow_files_per_s"] = spread(ref) if why is None else why
                        res["write"].append(row)
                        print("%dx%d B=%d %-8s %6d bytes: encode %.1f us (events) %.1f us (host clock); files/s device %s, Pillow %s" % (
                            H, W, B, name, nbytes, ev_us, host_us, row["device_files_per_s"]["runs"],
                            row["pillow_files_per_s"]["runs"] if why is None else why), flush=True)
        if a.no_stream_leg:
            res["stream"] = "not measured: --no-stream-leg"
        else:
            res["stream"] = stream_leg(os.path.join(tmp, "stream"), a.stream_frames, a.repeats)
            print("stream:", json.dumps(res["stream"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
