#!/usr/bin/env python3
"""Per-layer conv times of the frame program that bench.py times (one tick: batch = --frames-per-launch items of --height x --width), in
the mixed and the mxfp8 modes (GPU only):

    python tools/frame_conv_bench.py [--iters 20] [--out profiles/mxfp8_frame_convs.tsv]

Every op of the program is launched --iters times (eager, HIP events between the ops: Program.time(per_op=True)), so every conv signature
is timed over at least 20 launches.  Rows: one per conv layer (first key of the launch) with its signature, tiling and arithmetic in each
mode and the microseconds per launch; then the operand-preparation launches of each mode (split / quant) and the totals."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def per_op(mode, args, dev):
    os.environ["VIDC_PRECISION"] = mode      # engine.Program reads the mode when the program is recorded
    pipe = bench.build_pipeline(args.height, args.width, dev)[0]
    fp = pipe.frame_program(args.frames_per_launch, args.height, args.width)
    fp.time(iters=3, use_graph=False, per_op=True)                      # warm-up: code objects, caches
    total, per = fp.time(iters=args.iters, use_graph=False, per_op=True)
    return total, list(zip(fp.op_names, per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--frames-per-launch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--modes", default="mixed,mxfp8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    modes = args.modes.split(",")
    layers, prep, totals = {}, {}, {}
    for mode in modes:
        total, ops = per_op(mode, args, dev)
        conv_ms = 0.0
        for name, ms in ops:
            kind = name.split(":", 1)[0]
            if kind == "conv":
                _c, key, tile, _sk, rest = name.split(":", 4)
                arith, sig = rest.split(" ")[:2]
                layers.setdefault(key.split("@")[0], {})[mode] = (sig, tile, arith, ms * 1e3)
                conv_ms += ms
            elif kind in ("split", "quant", "wino_in", "wino_out"):
                prep.setdefault((mode, kind), [0, 0.0])
                prep[(mode, kind)][0] += 1
                prep[(mode, kind)][1] += ms * 1e3
        totals[mode] = {"program_ms_eager": round(total, 3), "conv_ms": round(conv_ms, 3)}
    lines = ["layer\t" + "\t".join("%s_signature\t%s_tile\t%s_arith\t%s_us" % (m, m, m, m) for m in modes)]
    for key in sorted(layers):
        row = [key]
        for m in modes:
            sig, tile, arith, us = layers[key].get(m, ("-", "-", "-", float("nan")))
            row += [sig, tile, arith, "%.2f" % us]
        lines.append("\t".join(row))
    for (m, kind), (n, us) in sorted(prep.items()):
        lines.append("# %s: %d %s launches, %.1f us" % (m, n, kind, us))
    lines.append("# totals per tick of %d items: %s" % (args.frames_per_launch, json.dumps(totals)))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
