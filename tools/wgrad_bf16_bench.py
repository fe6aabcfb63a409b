#!/usr/bin/env python3
"""The two conv weight-gradient entries side by side: vidc_conv_wgrad / vidc_conv_wgrad_dilated (fp32 operands on v_mfma_f32_32x32x2_f32, no LDS)
and vidc_conv_wgrad_bf16 (operands rounded to bf16 on the way into LDS, v_mfma_f32_32x32x16_bf16 behind transposed LDS reads), in one process, at
batch 8 on the layer shapes the autograd steps spend their weight-gradient time in.  Each time is one call of the entry -- the weight-gradient
kernel plus the shared final reduction -- between two HIP events: 5 warm-up calls, then the median of 25.  The operands (up to 157 MB) are the same
buffers in every call, so they are as warm as the 256 MB last-level cache keeps them; both entries see the same.

    python tools/wgrad_bf16_bench.py                  # the table, then one JSON line
    python tools/wgrad_bf16_bench.py --dgrad          # the DATA gradient instead: ops.conv_backward_data at precision 0 and 2

--dgrad times the whole wrapper call as the backward operator makes it -- weight packing (precision 2: the batched packer with its descriptor
upload), the bf16 cast of dc, the conv kernel -- between HIP events, and beside it the host's wall time per call while the GPU is kept busy
(the eager step is bound by that).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (layer, Cin, Cout, k, dilation, H, W) at 240 x 320 inputs
SHAPES = [("stem conv1_2", 64, 64, 3, 1, 120, 160),
          ("layer1 conv2", 64, 64, 3, 1, 60, 80),
          ("layer3 conv2", 256, 256, 3, 1, 15, 20),
          ("layer3 conv1", 1024, 256, 1, 1, 15, 20),
          ("layer4 conv2", 512, 512, 3, 1, 8, 10),
          ("ModifiedFPN feature1_upsamping.0", 768, 768, 3, 1, 60, 80),
          ("DORN ASPP d12", 2048, 512, 3, 12, 30, 40)]


def median_us(launch, n=25, warm=5):
    import torch
    times = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        if i >= warm:
            times.append(1e3 * e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def host_us(launch, n=25, warm=5):
    """Host wall time per call of `n` back-to-back calls (the stream runs behind; one synchronize at the end, not timed per call)."""
    import time
    import torch
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        launch()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1e6 * dt / n


def dgrad_table(B):
    import torch
    from vi_depth_completion_amd import ops
    dev = torch.device("cuda", 0)
    rows = []
    print("%-34s %12s %5s %9s %10s %10s %6s %10s %10s" % ("layer", "Cin -> Cout", "k", "map", "fp32 us", "bf16 us", "ratio", "host fp32", "host bf16"))
    for name, ci, co, k, d, H, W in SHAPES:
        pad = d * (k - 1) // 2
        g = torch.Generator().manual_seed(ci + co + k)
        w = (torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5).to(dev)
        dc = torch.randn(B, H, W, co, generator=g).to(dev)
        assert ops.conv_backward_data_precision((co, ci, k, k), 2) == 2
        f = {p: (lambda p=p: ops.conv_backward_data(dc, w, H, W, 1, pad, p, d)) for p in (0, 2)}
        t = {p: median_us(f[p]) for p in (0, 2)}
        h = {p: host_us(f[p]) for p in (0, 2)}
        rows.append({"layer": name, "Cin": ci, "Cout": co, "k": k, "dilation": d, "map": [H, W], "fp32_us": round(t[0], 1), "bf16_us": round(t[2], 1),
                     "fp32_over_bf16": round(t[0] / t[2], 2), "host_fp32_us": round(h[0], 1), "host_bf16_us": round(h[2], 1)})
        print("%-34s %12s %5s %9s %10.1f %10.1f %6.2f %10.1f %10.1f" % (name, "%d -> %d" % (ci, co), "%dx%d%s" % (k, k, " d%d" % d if d > 1 else ""),
                                                                         "%dx%d" % (H, W), t[0], t[2], t[0] / t[2], h[0], h[2]))
        del w, dc
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "conv data gradient, one ops.conv_backward_data call (pack + cast + conv)", "unit": "us", "batch": B, "shapes": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dgrad", action="store_true", help="time ops.conv_backward_data at precision 0 and 2 instead of the weight-gradient entries")
    args = ap.parse_args()
    if args.dgrad:
        return dgrad_table(args.batch)
    import torch
    from vi_depth_completion_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", 0)
    B = args.batch
    rows = []
    print("%-34s %12s %5s %9s %11s %11s %7s" % ("layer", "Cin -> Cout", "k", "map", "fp32 us", "bf16 us", "ratio"))
    for name, ci, co, k, d, H, W in SHAPES:
        pad = d * (k - 1) // 2
        g = torch.Generator().manual_seed(ci + co + k)
        x = torch.randn(B, H, W, ci, generator=g).to(dev)
        dy = torch.randn(B, H, W, co, generator=g).to(dev)
        dw32, dw16 = torch.empty(co, ci, k, k, device=dev), torch.empty(co, ci, k, k, device=dev)
        sc32 = torch.empty(lib.vidc_conv_wgrad_dilated_scratch_bytes(B, H, W, co, ci, k, k) + 256, dtype=torch.uint8, device=dev)
        sc16 = torch.empty(lib.vidc_conv_wgrad_bf16_scratch_bytes(B, H, W, co, ci, k, k) + 256, dtype=torch.uint8, device=dev)
        st = L.current_stream()
        if d == 1:
            f32 = lambda: L.check(lib.vidc_conv_wgrad(L.ptr(dy), L.ptr(x), L.ptr(dw32), B, H, W, ci, ci, H, W, co, co, k, k, 1, pad, L.ptr(sc32), st), "conv_wgrad")
        else:
            f32 = lambda: L.check(lib.vidc_conv_wgrad_dilated(L.ptr(dy), L.ptr(x), L.ptr(dw32), B, H, W, ci, ci, H, W, co, co, k, k, 1, pad, d, L.ptr(sc32), st),
                                  "conv_wgrad_dilated")
        b16 = lambda: L.check(lib.vidc_conv_wgrad_bf16(L.ptr(dy), L.ptr(x), L.ptr(dw16), B, H, W, ci, ci, H, W, co, co, k, k, 1, pad, d, L.ptr(sc16), st),
                              "conv_wgrad_bf16")
        t32, t16 = median_us(f32), median_us(b16)
        rel = float((dw16 - dw32).norm() / dw32.norm())
        rows.append({"layer": name, "Cin": ci, "Cout": co, "k": k, "dilation": d, "map": [H, W], "fp32_us": round(t32, 1), "bf16_us": round(t16, 1),
                     "fp32_over_bf16": round(t32 / t16, 2), "rel_l2_difference": float("%.3g" % rel)})
        print("%-34s %12s %5s %9s %11.1f %11.1f %7.2f" % (name, "%d -> %d" % (ci, co), "%dx%d%s" % (k, k, " d%d" % d if d > 1 else ""), "%dx%d" % (H, W), t32, t16,
                                                          t32 / t16))
        del x, dy, dw32, dw16, sc32, sc16
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "conv weight gradient, one call (kernel + final reduction)", "unit": "us", "batch": B, "shapes": rows}))


if __name__ == "__main__":
    main()
