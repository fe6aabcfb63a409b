"""Times the mixed, the mxfp8 and the bf16 inference modes (VIDC_LEG_MODES=mixed,bf16 picks some) in ONE process with bench.py's contract (bench.parse / bench.measure: --mode
interleaved, --frames-per-launch 4, 3 lanes, median of --regions 5 timed regions of --steps K steps) and prints one JSON line per mode,
with the relative depth RMSE of one frame against the fp32 path and, for the bf16 mode, the cast launches left per tick.  bench.py itself
times fp32 and mixed only.

    python tools/precision_leg.py --gpus 1 --steps 20 --warmup 5
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vi_depth_completion_amd import synthetic as S  # noqa: E402


def frame0_depth(args, dev, precision):
    """Depth of synthetic frame 0 through _call_cnn in `precision` (programs are recorded under VIDC_PRECISION)."""
    os.environ["VIDC_PRECISION"] = precision
    pipe = bench.build_pipeline(args.height, args.width, dev)[0]
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in S.synthetic_batch(args.batch, args.height, args.width, 1234).items()}
    pipe.rng = np.random.RandomState(7)
    return pipe._call_cnn(batch).double().cpu(), cast_launches(pipe, args, dev)


def cast_launches(pipe, args, dev):
    """Stand-alone cast launches (vidc_cast_bf16) in one tick program of the current mode: a dry-run recording at the bench shape."""
    from vi_depth_completion_amd.pipeline import build_frame_program
    prog = build_frame_program(pipe.surface_normal_cnn, pipe.cnn, args.batch * max(args.frames_per_launch, 1), args.height, args.width, dev, dry_run=True)
    return sum(1 for kind, _r, _w, _kw in prog.ops if kind == "cast")


def main():
    args = bench.parse()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ref = frame0_depth(args, dev, "fp32")[0]
    modes = [m for m in os.environ.get("VIDC_LEG_MODES", "mixed,mxfp8,bf16").split(",") if m]
    assert all(m in ("mixed", "mxfp8", "bf16") for m in modes), modes
    for mode in modes:
        res = bench.measure(args, dev, 0, 1, mode)
        regions = sorted(res["region_s"])
        d, n_cast = frame0_depth(args, dev, mode)
        rel = float((d - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        print(json.dumps({"metric": "frames/sec", "precision_mode": mode, "value": round(args.steps * args.batch / regions[len(regions) // 2], 3),
                          "unit": "frames/s", "steps": args.steps, "warmup": args.warmup, "frames_per_launch": args.frames_per_launch,
                          "lanes": res["lanes"], "regions_s": [round(r, 4) for r in res["region_s"]],
                          "depth_rel_rmse_vs_fp32_frame0": rel, "cast_launches_per_tick": n_cast}), flush=True)


if __name__ == "__main__":
    main()
