#!/usr/bin/env python3
"""Rate of the device-side training batches (ScanNetFramePreprocessor / NYUFramePreprocessor, csrc/train_preprocess.hip) against the host
restatement of the reference's two loaders (tests/train_preprocess_ref.py: PIL / numpy / torch CPU, one process), and what building the
next batch on a second stream costs the depth-completion training step of tools/train_bench.py.

    python tools/train_loader_bench.py                                  # all three legs, batch 8
    python tools/train_loader_bench.py --legs device --iters 500        # the device rates only
    python tools/train_loader_bench.py --legs host --host-batches 5     # the host restatement only (needs no GPU)

Inputs are seeded synthetic "decoded files": 8-bit colour / orientation / mask / predicted-normal images, 16-bit depth, a gravity vector and
--tracks pixel tracks per frame.  Device rates are wall clock over --iters batches between two device synchronisations, after --warmup
batches, once from host arrays (pinned upload included) and once from arrays already on the device.  The step leg alternates "step alone"
and "step + one batch built on a second stream per step" (A B A B) so that drift shows.  One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_files(B, seed, tracks, hw=(240, 320), nyu_hw=(480, 640)):
    """What the two loaders read from disk for B frames, decoded."""
    rng = np.random.RandomState(seed)
    H, W = hw
    u8 = lambda *s: rng.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    depth = rng.randint(300, 6000, (B, H, W)).astype(np.uint16)
    depth[rng.uniform(size=depth.shape) < 0.3] = 0
    g = rng.normal(size=(B, 3)) * 0.1 + np.array([0.0, 0.97, 0.24])
    tr = [np.stack([np.arange(tracks, dtype=np.float64), rng.uniform(0, 2 * W, tracks), rng.uniform(0, 2 * H, tracks), rng.uniform(0.5, 5.0, tracks)], axis=1)
          for _ in range(B)]
    scannet = dict(color=u8(B, H, W, 3), depth=depth, orient=u8(B, H, W, 3), mask=(rng.randint(0, 2, (B, H, W)) * 255).astype(np.uint8), gravity=g,
                   tracks=tr, pred=u8(B, H, W, 3))
    nyu = dict(color=u8(B, *nyu_hw, 3), depth=rng.randint(0, 40000, (B,) + tuple(nyu_hw)).astype(np.uint16), tracks=tr, pred=u8(B, H, W, 3))
    return scannet, nyu


def emit(**kw):
    print(json.dumps(kw), flush=True)


def host_leg(args, scannet, nyu):
    import train_preprocess_ref as R
    B = args.batch
    hom = R.homogeneous_coordinates(R.SCANNET_FC, R.SCANNET_CC, 320, 240)      # (the loader builds it once, in __init__)
    legs = {
        "scannet": lambda: R.collate([R.scannet_item(scannet["color"][b], scannet["depth"][b], scannet["orient"][b], scannet["mask"][b], scannet["gravity"][b],
                                                     scannet["tracks"][b], scannet["pred"][b], homogeneous=hom) for b in range(B)]),
        "scannet random sparse": lambda: R.collate([R.scannet_item(scannet["color"][b], scannet["depth"][b], scannet["orient"][b], scannet["mask"][b],
                                                                   scannet["gravity"][b], scannet["tracks"][b], scannet["pred"][b], random_sparse_pointcloud=True,
                                                                   rng=np.random.RandomState(1), homogeneous=hom) for b in range(B)]),
        "nyu": lambda: R.collate([R.nyu_item(nyu["color"][b], nyu["depth"][b], nyu["tracks"][b], nyu["pred"][b]) for b in range(B)]),
    }
    for name, fn in legs.items():
        fn()
        t0 = time.perf_counter()
        for _ in range(args.host_batches):
            fn()
        dt = time.perf_counter() - t0
        emit(metric="host restatement frames/sec", loader=name, value=round(B * args.host_batches / dt, 1), unit="frames/s", batch=B,
             ms_per_batch=round(1e3 * dt / args.host_batches, 2), batches=args.host_batches, tracks_per_frame=args.tracks,
             config="PIL / numpy / torch CPU, one process, decoded arrays in memory (no file reads, no PNG decode)")


def _rate(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _on_device(d, dev):
    up = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)      # noqa: E731
    return {k: (up(v) if isinstance(v, np.ndarray) and v.dtype in (np.uint8, np.uint16) else v) for k, v in d.items()}


def device_legs(args, scannet, nyu, dev):
    from vi_depth_completion_amd.preprocess import NYUFramePreprocessor, ScanNetFramePreprocessor
    B = args.batch
    sn_pre = ScanNetFramePreprocessor(dev)
    sn_rand = ScanNetFramePreprocessor(dev, generate_random_sparse_pointcloud=True, rng=np.random.RandomState(1))
    ny_pre = NYUFramePreprocessor(dev)
    call_sn = lambda pre, d: pre(d["color"], d["depth"], d["orient"], d["mask"], d["gravity"], d["tracks"], predicted_normal_u8=d["pred"])      # noqa: E731
    call_ny = lambda d: ny_pre(d["color"], d["depth"], d["tracks"], predicted_normal_u8=d["pred"])      # noqa: E731
    for src, sd, nd in (("host arrays (pinned upload included)", scannet, nyu), ("device arrays", _on_device(scannet, dev), _on_device(nyu, dev))):
        for name, fn in (("scannet", lambda: call_sn(sn_pre, sd)), ("scannet random sparse", lambda: call_sn(sn_rand, sd)), ("nyu", lambda: call_ny(nd))):
            dt = _rate(fn, args.warmup, args.iters)
            emit(metric="device loader frames/sec", loader=name, inputs=src, value=round(B * args.iters / dt, 1), unit="frames/s", batch=B,
                 ms_per_batch=round(1e3 * dt / args.iters, 3), batches=args.iters, tracks_per_frame=args.tracks)


def step_leg(args, scannet, dev):
    """tools/train_bench.py's depth step alone, and with one ScanNet batch per step built on a second stream (from host arrays)."""
    from vi_depth_completion_amd import synthetic as S
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.preprocess import ScanNetFramePreprocessor
    from vi_depth_completion_amd.training import DepthCompletionTrainer
    torch.set_grad_enabled(False)
    B = args.batch
    cnn = ModifiedFPN().to(dev)
    cnn.load_state_dict(S.seeded_state_dict(cnn.state_dict(), 1234, device=dev))
    cnn.train()
    tr = DepthCompletionTrainer(cnn, 1e-4)
    b = S.synthetic_batch(B, 240, 320, 1234)
    image = b["image"].to(dev)
    normal = torch.nn.functional.normalize(image - 0.5, dim=1)
    depth_in = b["sparse_depth"].to(dev)
    gt = S.synthetic_ground_truth_depth(b["image"], 1234).to(dev)
    pre = ScanNetFramePreprocessor(dev)
    side = torch.cuda.Stream(device=dev)

    def build():
        with torch.cuda.stream(side):
            return pre(scannet["color"], scannet["depth"], scannet["orient"], scannet["mask"], scannet["gravity"], scannet["tracks"], predicted_normal_u8=scannet["pred"])

    def alone():
        tr.step(image, normal, depth_in, gt)

    def with_loader():
        build()
        tr.step(image, normal, depth_in, gt)

    for _ in range(args.step_warmup):
        with_loader()
    ms = {"alone": [], "with_loader": []}
    for _ in range(2):
        for name, fn in (("alone", alone), ("with_loader", with_loader)):
            ms[name].append(round(1e3 * _rate(fn, 1, args.steps) / args.steps, 2))
    emit(metric="depth training step with the next batch built on a second stream", unit="ms/step", batch=B, steps=args.steps, order="A B A B",
         step_alone_ms=ms["alone"], step_with_loader_ms=ms["with_loader"], dtype=os.environ.get("VIDC_TRAIN_PRECISION", "fp32"),
         config="DepthCompletionTrainer.step as in tools/train_bench.py; ScanNetFramePreprocessor from host arrays on a second stream, one batch per step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tracks", type=int, default=2000, help="tracks per frame (an observed point cloud holds thousands)")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-batches", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--legs", default="host,device,step")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    scannet, nyu = synthetic_files(args.batch, 1234, args.tracks)
    if "host" in legs:
        host_leg(args, scannet, nyu)
    if legs & {"device", "step"}:
        if not torch.cuda.is_available():
            raise RuntimeError("the device and step legs need a GPU: there is no CPU path to time")
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        if "device" in legs:
            device_legs(args, scannet, nyu, dev)
        if "step" in legs:
            step_leg(args, scannet, dev)


if __name__ == "__main__":
    main()
