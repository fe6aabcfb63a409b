#!/usr/bin/env python3
"""Timing of the backward of the scene-understanding module's operators at SurfaceNormalDORN's own shapes, in one process, in the style of
tools/warp_backward_bench.py (HIP events around one call, 5 warm-up calls, median of 25):
  conv2d_dilated_bn_act at B = 8, 30 x 40, 2048 -> 512, dilation 6 / 12 / 18 in fp32: the forward conv against the three parts of its backward
  (vidc_affine_act_backward, the data gradient = the same conv kernel on data-gradient weights, vidc_conv_wgrad_dilated);
  vidc_avgpool2d_backward at B = 8, 30 x 40 x 2048, AvgPool2d(8, 8, padding=(1, 0)), against the bytes it moves (dx written + dy read once).
Weights are packed outside the timed region.  GPU only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vi_depth_completion_amd import _lib as L, ops, synthetic as S      # noqa: E402


def median_us(launch, n=25, warm=5):
    ts = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    lib = L.lib()
    B, H, W, ci, co = 8, 30, 40, 2048, 512
    M = B * H * W
    x = S.normal01(6, "bench.x", (B, H, W, ci)).float().cuda()
    w = (S.normal01(6, "bench.w", (co, ci, 3, 3)).float() * (2.0 / (ci * 9)) ** 0.5).cuda()
    scale, shift = (0.5 + S.uniform01(6, "bench.s", (co,)).float()).cuda(), (0.1 * S.normal01(6, "bench.b", (co,)).float()).cuda()
    one, zero = torch.ones(ci, device="cuda"), torch.zeros(ci, device="cuda")
    dy = S.normal01(6, "bench.dy", (B, H, W, co)).float().cuda()
    wf, wd = ops.pack_conv_weight(w), ops.pack_conv_weight_dgrad(w, 0)
    dw = torch.empty_like(w)
    sc_w = torch.empty(lib.vidc_conv_wgrad_dilated_scratch_bytes(B, H, W, co, ci, 3, 3) + 256, dtype=torch.uint8, device="cuda")
    sc_a = torch.empty(lib.vidc_train_scratch_bytes(M, co) + 256, dtype=torch.uint8, device="cuda")
    dc, ds, db = torch.empty_like(dy), torch.empty_like(scale), torch.empty_like(shift)
    flop = 2.0 * M * co * ci * 9
    print("%-34s %9s %9s %9s %9s %9s %8s" % ("conv2d_dilated_bn_act 2048->512", "fwd us", "affine us", "dgrad us", "wgrad us", "bwd/fwd", "fwd TF/s"))
    for d in (6, 12, 18):
        y = ops.conv2d_bn_act(x, wf, scale, shift, 3, 3, pad=d, relu1=True, dilation=d)
        tf = median_us(lambda: ops.conv2d_bn_act(x, wf, scale, shift, 3, 3, pad=d, relu1=True, dilation=d))
        ta = median_us(lambda: lib.vidc_affine_act_backward(L.ptr(dy), L.ptr(y), None, L.ptr(scale), L.ptr(shift), L.ptr(dc), L.ptr(ds), L.ptr(db), M, co, co, co,
                                                            co, co, 1, L.ptr(sc_a), L.current_stream()))
        tx = median_us(lambda: ops.conv2d_bn_act(dc, wd, one, zero, 3, 3, pad=d, dilation=d))
        tw = median_us(lambda: lib.vidc_conv_wgrad_dilated(L.ptr(dc), L.ptr(x), L.ptr(dw), B, H, W, ci, ci, H, W, co, co, 3, 3, 1, d, d, L.ptr(sc_w),
                                                           L.current_stream()))
        print("%-34s %9.1f %9.1f %9.1f %9.1f %9.2f %8.1f" % ("B=8 30x40 dilation %d" % d, tf, ta, tx, tw, (ta + tx + tw) / tf, flop / tf * 1e-6))
    Ho, Wo = (H + 2 - 8) // 8 + 1, (W - 8) // 8 + 1
    g = S.normal01(6, "bench.pool", (B, Ho, Wo, ci)).float().cuda()
    dx = torch.empty_like(x)
    tp = median_us(lambda: lib.vidc_avgpool2d_backward(L.ptr(g), L.ptr(dx), B, H, W, ci, ci, 8, 8, 8, 8, 1, 0, ci, L.current_stream()))
    nbytes = (dx.numel() + g.numel()) * 4
    print("vidc_avgpool2d_backward B=8 30x40x2048 k8 s8 p(1,0): %.1f us, %.1f MB moved, %.0f GB/s" % (tp, nbytes * 1e-6, nbytes / tp * 1e-3))


if __name__ == "__main__":
    main()
