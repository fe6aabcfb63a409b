#!/usr/bin/env python3
"""One training step of ModifiedFPN (--net depth), SurfaceNormalPrediction (--net normal) or SurfaceNormalDORN (--net dorn) under autograd:
forward_autograd + the loss operator + backward() + torch.optim.Adam.step(), the reference's loop (network_run.py:231-254), at batch 8, 240x320 -- eager, at
precision 0 (exact fp32 convs) and 1 (bf16x3 forward) -- with the matching trainer's captured step (DepthCompletionTrainer / SurfaceNormalTrainer, in the
arithmetic VIDC_TRAIN_PRECISION selects; SurfaceNormalDORN has no trainer) timed beside it in the same process on the same inputs.  Timed like
tools/train_bench.py: `--warmup` untimed steps, then wall clock over `--steps` steps (host enqueue time and time to the last kernel), and by HIP events the
three regions of an autograd step: forward + loss, backward, Adam.

    python tools/net_train_step_bench.py --net depth --batch 8 --steps 5                          # one JSON line
    python tools/net_train_step_bench.py --net normal --batch 8 --use-mask                        # SurfaceNormalPrediction(use_mask=True): autograd only
    python tools/net_train_step_bench.py --net dorn --batch 8 --precisions 0                      # SurfaceNormalDORN, dropout_seed 1234: autograd only
    python tools/net_train_step_bench.py --net normal --precisions 0 --no-trainer --frozen-bn all # fine-tuning with frozen BatchNorm beside the train-mode step
    python tools/net_train_step_bench.py --net depth --precisions 0 --grad-precisions 0,2         # ... and with plain-bf16 conv gradients (grad_precision=2)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o net -- python tools/net_train_step_bench.py --net depth --precisions 0 --no-trainer
    python tools/net_train_step_bench.py --kernel-stats OUT/.../net_kernel_stats.csv              # the per-kernel share table of that run (no GPU needed)

The share table groups the kernels of the profiled process (warm-up steps included: they are the same steps) into what the step spends its GPU
time on -- convs, BatchNorm passes, per-call weight packing, weight-gradient operands, the transposed conv epilogue, torch's own kernels (Adam, cat,
zero_grad) -- and lists the kernels above 1 %.

--frozen-bn backbone|all puts the BatchNorm2d modules of the ResNet backbones / of the whole network into eval() mode (fine-tuning with frozen BatchNorm:
batch_norm_eval instead of batch_norm_train) and times that step beside the train-mode one ("none", today's step) in the same process on the same inputs,
each with the share of the step's GPU time its BatchNorm operators take, forward and backward (HIP events around the four operators' entry points in
`--steps` further steps, so the timed steps carry no extra events)."""
import argparse
import csv
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = {0: "f32 (fp32 MFMA fwd / dgrad / wgrad)", 1: "f32+bf16x3 forward, fp32 dgrad / wgrad"}
GRAD_DTYPES = {0: "f32 forward, bf16 dgrad / wgrad", 1: "f32+bf16x3 forward, bf16 dgrad / wgrad"}      # grad_precision 2
NETS = {"depth": ("ModifiedFPN", "depth_l1_loss"), "normal": ("SurfaceNormalPrediction", "normal_l1_loss"), "dorn": ("SurfaceNormalDORN", "normal_l1_loss")}

BACKBONES = ("resnet_rgb.", "resnet_normal.", "resnet_depth.", "resnet_pyramids.", "feature_extractor.")
BN_ENTRIES = ("batch_norm_train", "batch_norm_train_backward", "batch_norm_eval", "batch_norm_eval_backward")      # of vi_depth_completion_amd.ops

GROUPS = (("BatchNorm passes", ("chan_partial_kernel", "chan_final_kernel", "bn_apply", "bn_bwd_apply", "bn_eval_")),
          ("per-call weight packing", ("pack_weight", "pack_batched_kernel", "pack_one_kernel")),
          ("weight-gradient operands / permute", ("im2col_t", "wgrad_permute_kernel", "transpose_bf16_kernel")),
          ("transposed conv epilogue", ("affine_act_bwd_kernel",)),
          ("ReLU mask / residual gradient", ("relu_bwd_kernel",)),
          ("data-gradient zero stuffing", ("zero_stuff_kernel",)),
          ("dropout, normalize, loss", ("dropout2d_mask_kernel", "scale_image_channels_kernel", "normalize_nchw", "normal_loss")),
          ("stem, pools, upsample, head", ("stem_", "maxpool", "avgpool", "upsample", "head_")),
          ("torch (Adam, cat, zero_grad, fills)", ("at::", "elementwise_kernel", "Memset", "Copy", "multi_tensor")),
          ("convs (forward, data gradient, weight-gradient GEMM)", ("conv", "wgemm", "wgrad", "wino")))


def share_table(path):
    rows = [(r["Name"].replace("(anonymous namespace)::", ""), int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    total = sum(t for _, _, t in rows)
    sums = {g: [0, 0.0] for g, _ in GROUPS}
    sums["other"] = [0, 0.0]
    for name, calls, t in rows:
        g = next((g for g, keys in GROUPS if any(k in name for k in keys)), "other")
        sums[g][0] += calls
        sums[g][1] += t
    print("%-56s %9s %11s %7s" % ("group", "calls", "total ms", "%"))
    for g, (calls, t) in sorted(sums.items(), key=lambda kv: -kv[1][1]):
        print("%-56s %9d %11.2f %7.1f" % (g, calls, t / 1e6, 100.0 * t / total))
    print("\n%-88s %9s %11s %7s %9s" % ("kernel (above 1 %)", "calls", "total ms", "%", "avg us"))
    for name, calls, t in sorted(rows, key=lambda r: -r[2]):
        if t < 0.01 * total:
            break
        print("%-88s %9d %11.2f %7.1f %9.1f" % (name.split("(")[0][:88], calls, t / 1e6, 100.0 * t / total, t / calls / 1e3))
    print("total: %.1f ms of kernel time in the profiled process" % (total / 1e6))


def timed(step, steps, warmup, events=None):
    """(ms per step, host enqueue ms per step, losses) of `steps` calls of step(marks) after `warmup` untimed ones."""
    import torch
    warm = [round(float(step(None)), 6) for _ in range(warmup)]
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        losses.append(step(events[i] if events is not None else None))
    t_enq = time.perf_counter() - t0          # host time to enqueue the steps (the GPU runs behind it when the step is GPU-bound)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return 1e3 * dt / steps, 1e3 * t_enq / steps, warm + [round(float(x), 6) for x in losses]


def freeze_batch_norms(cnn, which):
    """--frozen-bn: eval() on the BatchNorm2d modules of the backbones ("backbone") or of the whole network ("all"); the count."""
    import torch
    n = 0
    for name, m in cnn.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and (which == "all" or name.startswith(BACKBONES)):
            m.eval()
            n += 1
    return n


def batch_norm_share(step, steps):
    """(ms per step inside the BatchNorm operators, share of the step's GPU time): `steps` further steps with a HIP event pair around every call of the
    BatchNorm entry points of vi_depth_completion_amd.ops (the stream is in order: a pair brackets exactly the kernels the call launched)."""
    import torch
    from vi_depth_completion_amd import ops
    pairs, real = [], {n: getattr(ops, n) for n in BN_ENTRIES}

    def bracket(fn):
        def call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            pairs.append((e0, e1))
            return r
        return call

    ends = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for n, fn in real.items():
        setattr(ops, n, bracket(fn))
    try:
        ends[0].record()
        for _ in range(steps):
            step(None)
        ends[1].record()
        torch.cuda.synchronize()
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)
    bn_ms = sum(a.elapsed_time(b) for a, b in pairs)
    return round(bn_ms / steps, 2), round(bn_ms / ends[0].elapsed_time(ends[1]), 4), len(pairs) // steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=tuple(NETS), default="depth")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precisions", default="0,1", help="the convs' arithmetic of the autograd steps to time: 0 exact fp32, 1 bf16x3 (default: both)")
    ap.add_argument("--grad-precisions", default="0",
                    help="the conv gradients' arithmetic of the autograd steps to time: 0 fp32, 2 plain bf16 (forward_autograd's grad_precision; default: 0)")
    ap.add_argument("--use-mask", action="store_true", help="--net normal: SurfaceNormalPrediction(use_mask=True), which only the autograd step trains")
    ap.add_argument("--frozen-bn", choices=("none", "backbone", "all"), default="none",
                    help="BatchNorm2d modules to put into eval() mode (frozen); not none: the train-mode step is timed beside it, both with their BatchNorm share")
    ap.add_argument("--no-trainer", action="store_true", help="skip the trainer's step (a profile of the autograd step alone)")
    ap.add_argument("--kernel-stats", help="a rocprofv3 --kernel-trace --stats CSV of a run of this script: print its share table and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return share_table(args.kernel_stats)
    import torch
    from vi_depth_completion_amd import synthetic as S
    from vi_depth_completion_amd import torch_ops  # noqa: F401  (registers torch.ops.vidc)
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction
    from vi_depth_completion_amd.networks.surface_normal_dorn import SurfaceNormalDORN
    from vi_depth_completion_amd.training import DepthCompletionTrainer, SurfaceNormalTrainer
    V = torch.ops.vidc
    dev = torch.device("cuda", 0)
    B = args.batch
    b = S.synthetic_batch(B, 240, 320, 1234)
    image = b["image"].to(dev)
    if args.net == "depth":
        make = ModifiedFPN
        inputs = (image, torch.nn.functional.normalize(image - 0.5, dim=1), b["sparse_depth"].to(dev))
        target = (S.synthetic_ground_truth_depth(b["image"], 1234).to(dev),)
        loss_of = lambda out: V.depth_l1_loss(out, *target)[0]
        forward_args = {}
    else:
        dorn = args.net == "dorn"
        make = (lambda: SurfaceNormalDORN(pretrained=False)) if dorn else (lambda: SurfaceNormalPrediction(use_mask=args.use_mask))
        inputs = (image,) if dorn else (image, b["gravity"].to(dev), b["aligned_direction"].to(dev))
        forward_args = {"dropout_seed": 1234} if dorn else {}
        target = ((S.normal01(1234, "sn.gt", (B, 3, 240, 320)).float() * 1.7).to(dev),
                  (S.uniform01(1234, "sn.mask", (B, 1, 240, 320) if dorn else (B, 240, 320)) < 0.7).float().to(dev))
        loss_of = lambda out: V.normal_l1_loss(out, *target, not dorn)[0]          # (SurfaceNormalDORN's output is normalized already)

    def network():
        cnn = make().to(dev)
        cnn.load_state_dict(S.seeded_state_dict(cnn.state_dict(), 1234))          # (drawn on the CPU: no generator kernels in a profile of the step)
        return cnn.train()

    result = {"metric": "%s autograd training step" % NETS[args.net][0], "unit": "ms/step", "n_gpus": 1,
              "batch_per_gpu": B, "use_mask": bool(args.use_mask), "autograd": {}}
    settings = ["none"] if args.frozen_bn == "none" else ["none", args.frozen_bn]
    grads = [int(g) for g in args.grad_precisions.split(",") if g != ""]
    for precision, grad, frozen in [(int(p), g, f) for p in args.precisions.split(",") if p != "" for g in grads for f in settings]:
        cnn = network()
        n_frozen = freeze_batch_norms(cnn, frozen) if frozen != "none" else 0
        optimizer = torch.optim.Adam(cnn.parameters(), lr=1e-4)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]

        def step(marks):
            mark = (lambda i: marks[i].record()) if marks is not None else (lambda i: None)
            mark(0)
            optimizer.zero_grad()
            loss = loss_of(cnn.forward_autograd(*inputs, precision=precision, **forward_args, **({"grad_precision": grad} if grad else {})))
            mark(1)
            loss.backward()
            mark(2)
            optimizer.step()
            mark(3)
            return loss.detach()

        torch.cuda.reset_peak_memory_stats()
        with torch.enable_grad():
            ms, enq, losses = timed(step, args.steps, args.warmup, ev)
        region = lambda a, c: round(sum(e[a].elapsed_time(e[c]) for e in ev) / args.steps, 2)
        key = (str(precision) if frozen == "none" else "%d frozen-bn=%s" % (precision, frozen)) + (" grad=%d" % grad if grad else "")
        result["autograd"][key] = {"ms_per_step": round(ms, 1), "frames_per_s": round(1e3 * B / ms, 1), "host_enqueue_ms_per_step": round(enq, 1),
                                   "forward_loss_ms": region(0, 1), "backward_ms": region(1, 2), "adam_ms": region(2, 3),
                                   "dtype": (GRAD_DTYPES if grad else DTYPES)[precision],
                                   "losses": losses, "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        if args.frozen_bn != "none":
            with torch.enable_grad():
                bn_ms, share, calls = batch_norm_share(step, args.steps)
            result["autograd"][key].update(frozen_batch_norms=n_frozen, batch_norm_ms=bn_ms, batch_norm_share=share, batch_norm_calls_per_step=calls)
            print("%s precision %d frozen-bn=%-8s %7.1f ms/step (forward+loss %.1f, backward %.1f), BatchNorm operators %.2f ms = %.1f %% of the step's GPU time"
                  % (NETS[args.net][0], precision, frozen, ms, region(0, 1), region(1, 2), bn_ms, 100 * share))
        del cnn, optimizer, step
        gc.collect()                            # (the module holds reference cycles: without this the next setting's peak memory counts this network too)
        torch.cuda.empty_cache()
    if not args.no_trainer and not args.use_mask and args.net != "dorn":
        with torch.no_grad():
            tr = (DepthCompletionTrainer if args.net == "depth" else SurfaceNormalTrainer)(network(), 1e-4)
            ms, enq, losses = timed(lambda _marks: tr.step(*inputs, *target), args.steps, max(args.warmup, 3))      # (the trainer captures its graph in its third step)
        result["trainer"] = {"ms_per_step": round(ms, 1), "frames_per_s": round(1e3 * B / ms, 1), "host_enqueue_ms_per_step": round(enq, 1),
                             "precision": os.environ.get("VIDC_TRAIN_PRECISION", "fp32"), "losses": losses}
        for p, r in result["autograd"].items():
            r["vs_trainer"] = round(r["ms_per_step"] / result["trainer"]["ms_per_step"], 2)
    result["config"] = "forward_autograd + %s + backward() + torch.optim.Adam.step(), eager, 320x240, synthetic" % NETS[args.net][1]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
