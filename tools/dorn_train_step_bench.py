#!/usr/bin/env python3
"""One training step of SurfaceNormalDORN under autograd: forward_autograd + normal_l1_loss + backward() + torch.optim.Adam.step(), the
reference's loop (network_run.py:231-254), at batch 8, 240x320.  Timed like tools/train_bench.py: `--warmup` untimed steps, then wall clock over
`--steps` steps (host enqueue time and time to the last kernel), and by HIP events the three regions of a step: forward + loss, backward, Adam.

    python tools/dorn_train_step_bench.py --batch 8 --steps 5                                     # one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o dorn -- python tools/dorn_train_step_bench.py --batch 8 --steps 5
    python tools/dorn_train_step_bench.py --kernel-stats OUT/.../dorn_kernel_stats.csv            # the per-kernel share table of that run (no GPU needed)

The share table groups the kernels of the profiled process (warm-up steps included: they are the same steps) into what the step spends its GPU
time on -- convs, BatchNorm passes, per-call weight packing, weight-gradient operands, the transposed conv epilogue, torch's own kernels (Adam, cat,
zero_grad) -- and lists the kernels above 1 %."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = (("BatchNorm passes", ("chan_partial_kernel", "chan_final_kernel", "bn_apply", "bn_bwd_apply")),
          ("per-call weight packing", ("pack_weight", "pack_batched_kernel")),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", type=int, default=0, choices=(0, 1), help="the convs' arithmetic: 0 exact fp32 (default), 1 bf16x3")
    ap.add_argument("--kernel-stats", help="a rocprofv3 --kernel-trace --stats CSV of a run of this script: print its share table and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return share_table(args.kernel_stats)
    import torch
    from vi_depth_completion_amd import synthetic as S
    from vi_depth_completion_amd import torch_ops  # noqa: F401  (registers torch.ops.vidc)
    from vi_depth_completion_amd.networks.surface_normal_dorn import SurfaceNormalDORN
    dev = torch.device("cuda", 0)
    cnn = SurfaceNormalDORN(pretrained=False).to(dev)
    cnn.load_state_dict(S.seeded_state_dict(cnn.state_dict(), 1234))          # (drawn on the CPU: no generator kernels in a profile of the step)
    cnn.train()
    optimizer = torch.optim.Adam(cnn.parameters(), lr=1e-4)
    B = args.batch
    image = S.synthetic_batch(B, 240, 320, 1234)["image"].to(dev)
    normal_gt = (S.normal01(1234, "sn.gt", (B, 3, 240, 320)).float() * 1.7).to(dev)
    mask = (S.uniform01(1234, "sn.mask", (B, 1, 240, 320)) < 0.7).float().to(dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]

    def step(marks=None):
        mark = (lambda i: marks[i].record()) if marks is not None else (lambda i: None)
        mark(0)
        optimizer.zero_grad()
        out = cnn.forward_autograd(image, dropout_seed=1234, precision=args.precision)
        loss, _count, _angle = torch.ops.vidc.normal_l1_loss(out, normal_gt, mask, False)
        mark(1)
        loss.backward()
        mark(2)
        optimizer.step()
        mark(3)
        return loss.detach()

    warm = [round(float(step()), 6) for _ in range(args.warmup)]
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        losses.append(step(ev[i]))
    t_enq = time.perf_counter() - t0          # host time to enqueue the steps (the GPU runs behind it when the step is GPU-bound)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    region = lambda a, b: round(sum(e[a].elapsed_time(e[b]) for e in ev) / args.steps, 2)
    print(json.dumps({"metric": "SurfaceNormalDORN autograd training frames/sec", "value": round(B * args.steps / dt, 2), "unit": "frames/s", "n_gpus": 1,
                      "batch_per_gpu": B, "ms_per_step": round(1e3 * dt / args.steps, 1), "host_enqueue_ms_per_step": round(1e3 * t_enq / args.steps, 1),
                      "forward_loss_ms": region(0, 1), "backward_ms": region(1, 2), "adam_ms": region(2, 3),
                      "dtype": {0: "f32 (fp32 MFMA fwd / dgrad / wgrad)", 1: "f32+bf16x3 forward, fp32 dgrad / wgrad"}[args.precision],
                      "losses": warm + [round(float(x), 6) for x in losses], "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                      "config": "SurfaceNormalDORN.forward_autograd + normal_l1_loss + backward() + torch.optim.Adam.step(), 320x240, synthetic"}))


if __name__ == "__main__":
    main()
