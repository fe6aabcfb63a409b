#!/usr/bin/env python3
"""Training throughput of the depth-completion network (BASELINE configs[4]: "Training loop: depth_completion.py L1 + normal loss,
batch=64 on 8xMI355X"): one `_run_training_iteration` per step (network_run.py:231-254) on this rank's share of the batch.

    python tools/train_bench.py --batch 8 --steps 5                                  # one GPU's share of batch 64
    python tools/train_bench.py --network sn --batch 8                               # the surface-normal network's step (one rank only)
    python tools/train_bench.py --network both --batch 8                             # both in one process, one JSON line each, and their ratio
    python tools/train_bench.py --weight-decay 0.01 --decoupled --max-grad-norm 1    # AdamW + clipping on the device (csrc/optim.hip)
    python tools/train_bench.py --accumulate 8                                       # a "step" is a window: 7 backward_only + 1 step (batch 8 x 8)
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... tools/train_bench.py --batch 8

Frames shard over ranks (weak scaling), BatchNorm statistics per rank (like the reference's DataParallel replicas), gradients
summed with a bucketed RCCL all-reduce of the flat 1.24 GB gradient buffer.  Prints one JSON line (rank 0)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vi_depth_completion_amd import synthetic as S  # noqa: E402
from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN  # noqa: E402
from vi_depth_completion_amd.networks.surface_normal import SurfaceNormalPrediction  # noqa: E402
from vi_depth_completion_amd.training import DepthCompletionTrainer, SurfaceNormalTrainer  # noqa: E402

PRECISIONS = {"fp32": "f32 (fp32 MFMA fwd / dgrad / wgrad)", "bf16x3": "f32+bf16x3 (split-bf16 3-pass MFMA fwd / dgrad / wgrad)",
              "bf16": "bf16 operands, fp32 accumulate (MFMA fwd / dgrad / wgrad); fp32 master weights, BatchNorm, loss, Adam"}


def optimizer_options(args):
    """The trainers' optimizer keywords from the command line; all defaults: the plain Adam launch."""
    return dict(weight_decay=args.weight_decay, decoupled_weight_decay=args.decoupled, max_grad_norm=args.max_grad_norm)


def window(tr, k, *ins):
    """One optimizer step over k micro-batches (the same data: a throughput tool): k - 1 `backward_only`, then the `step` that closes the window."""
    for _ in range(k - 1):
        tr.backward_only(*ins)
    return tr.step(*ins)


def optimizer_report(args, tr):
    """What the JSON line says about the options (nothing when they are at their defaults; ms_per_step is then the time of a whole window)."""
    if not (args.weight_decay or args.max_grad_norm is not None or args.accumulate > 1):
        return {}
    out = {"optimizer": dict(optimizer_options(args), accumulate=args.accumulate)}
    if tr.last_grad_norm is not None:
        out["last_grad_norm"] = float(tr.last_grad_norm)
    return out


def surface_normal_leg(args, dev):
    """The surface-normal step: seeded weights, synthetic gravity / normals / mask, timed like the depth leg (wall clock over `steps` steps
    after `warmup`); the loss kernel alone by HIP events over 20 calls."""
    from vi_depth_completion_amd import _lib as L
    cnn = SurfaceNormalPrediction().to(dev)
    cnn.load_state_dict(S.seeded_state_dict(cnn.state_dict(), 1234, device=dev))
    cnn.train()
    tr = SurfaceNormalTrainer(cnn, 1e-4, **optimizer_options(args))
    K = args.accumulate
    B = args.batch
    b = S.synthetic_batch(B, 240, 320, 1234)
    image, gravity, aligned = b["image"].to(dev), b["gravity"].to(dev), b["aligned_direction"].to(dev)
    normal_gt = (S.normal01(1234, "sn.gt", (B, 3, 240, 320)).float() * 1.7).to(dev)
    mask = (S.uniform01(1234, "sn.mask", (B, 240, 320)) < 0.7).float().to(dev)
    warm = [round(float(window(tr, K, image, gravity, aligned, normal_gt, mask)), 6) for _ in range(args.warmup)]
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(window(tr, K, image, gravity, aligned, normal_gt, mask))
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pred = torch.nn.functional.normalize(normal_gt + 0.3, dim=1)
    st, dp = torch.zeros(3, dtype=torch.float64, device=dev), torch.empty_like(pred)
    sc = torch.empty(L.lib().vidc_normal_l1_loss_scratch_bytes(B, 240, 320), dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(22):
        if i == 2:
            ev[0].record()
        L.check(L.lib().vidc_normal_l1_loss(L.ptr(pred), L.ptr(normal_gt), L.ptr(mask), B, 240, 320, 1, L.ptr(st), L.ptr(st[1:]), L.ptr(st[2:]), L.ptr(dp), L.ptr(sc),
                                            L.current_stream()), "normal loss")
    ev[1].record()
    torch.cuda.synchronize()
    ms = 1e3 * dt / args.steps
    print(json.dumps({"metric": "surface-normal training frames/sec", "value": round(K * B * args.steps / dt, 2), "unit": "frames/s", "n_gpus": 1, "batch_per_gpu": B,
                      "ms_per_step": round(ms, 1), "host_enqueue_ms_per_step": round(1e3 * t_enq / args.steps, 1),
                      "loss_kernel_ms": round(ev[0].elapsed_time(ev[1]) / 20, 4), "dtype": PRECISIONS[os.environ.get("VIDC_TRAIN_PRECISION", "fp32")],
                      "losses": warm + [round(float(x), 6) for x in losses], "angle_sum": round(float(tr.last_angle), 2), **optimizer_report(args, tr),
                      "config": "SurfaceNormalPrediction training step (train-mode BN, normal L1 / N, Adam), 320x240, synthetic"}))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--same-data", action="store_true", help="every rank trains on rank 0's frames: the summed gradient is N x the single-rank one and\n"
                                                             "Adam's update does not depend on the gradient's scale, so the losses must follow the single-rank run")
    ap.add_argument("--network", choices=("dc", "sn", "both"), default="dc", help="dc: the depth-completion network (default); sn: the surface-normal\n"
                                                                                 "network; both: one after the other in this process")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="torch.optim.Adam's weight_decay (L2), or with --decoupled torch.optim.AdamW's")
    ap.add_argument("--decoupled", action="store_true")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the gradient's global norm (torch.nn.utils.clip_grad_norm_); inf: measure only")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K", help="K micro-batches of --batch frames per optimizer step (K - 1 backward_only + 1 step);\n"
                                                                          "ms_per_step is then the time of the whole window")
    args = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.set_grad_enabled(False)
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("VIDC_DIST_BACKEND", "nccl")      # "nccl" is RCCL on ROCm; "gloo" to try the N > 1 path on a 1-GPU box
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    sn_ms = surface_normal_leg(args, dev) if args.network in ("sn", "both") else None      # (refuses a process group of more than one rank)
    if args.network == "sn":
        return
    cnn = ModifiedFPN().to(dev)
    cnn.load_state_dict(S.seeded_state_dict(cnn.state_dict(), 1234, device=dev))
    cnn.train()
    tr = DepthCompletionTrainer(cnn, 1e-4, **optimizer_options(args))
    K = args.accumulate
    B = args.batch
    b = S.synthetic_batch(B, 240, 320, 1234, frame0=0 if args.same_data else rank * B)
    image = b["image"].to(dev)
    normal = torch.nn.functional.normalize(image - 0.5, dim=1)
    depth_in = b["sparse_depth"].to(dev)
    gt = S.synthetic_ground_truth_depth(b["image"], 1234).to(dev)
    losses = []
    for _ in range(args.warmup):
        losses.append(window(tr, K, image, normal, depth_in, gt))
    warm = [round(float(x), 6) for x in losses]
    losses = []
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(window(tr, K, image, normal, depth_in, gt))
    t_enq = time.perf_counter() - t0          # host time to enqueue the steps (the GPU runs behind it when the step is GPU-bound)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if rank == 0:
        print(json.dumps({"metric": "training frames/sec", "value": round(world * K * B * args.steps / dt, 2), "unit": "frames/s", "n_gpus": world,
                          "batch_per_gpu": B, "ms_per_step": round(1e3 * dt / args.steps, 1), "host_enqueue_ms_per_step": round(1e3 * t_enq / args.steps, 1), "dtype": PRECISIONS[os.environ.get("VIDC_TRAIN_PRECISION", "fp32")],
                          "losses": warm + [round(float(x), 6) for x in losses], **optimizer_report(args, tr),
                          "config": "BASELINE configs[4]: ModifiedFPN training step (train-mode BN, masked L1 / (H*W), Adam), 320x240, synthetic"}))
        if sn_ms is not None:
            print(json.dumps({"metric": "surface-normal step / depth step", "value": round(sn_ms / (1e3 * dt / args.steps), 3), "sn_ms_per_step": round(sn_ms, 1),
                              "dc_ms_per_step": round(1e3 * dt / args.steps, 1)}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
