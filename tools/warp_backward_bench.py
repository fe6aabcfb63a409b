#!/usr/bin/env python3
"""Timing of the new backward kernels against the forward kernel of the same operator at the same shape, in one process: the two warp
adjoints (vidc_warp2dof_fwd_backward, vidc_warp2dof_inv_rot_norm_backward) at the program batch (1) and at batch 32, and the transposed
conv epilogue (vidc_affine_act_backward) at a ResNet-101 layer-3 shape (15 x 20 x 1024, batch 8) against vidc_relu_backward, the plain
two-reads-one-write pass over the same rows.  HIP events around ONE launch, inputs re-written by a device copy before every launch (as
tools/glue_bench.py does for single-use data), 5 warm-up launches, median of 25.  The forward warp kernels are the parent commit's,
instruction for instruction (the adjoints were added beside them), so the yardstick needs no second library.  Prints backward / forward
time ratio, achieved GB/s over the algorithmic bytes (input + output tensors once) and the candidate-window sizes the adjoints walk.
GPU only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vi_depth_completion_amd import _lib as L, ops, synthetic as S      # noqa: E402
from vi_depth_completion_amd.networks.warping_2dof_alignment import Warping2DOFAlignment      # noqa: E402

FX, FY, CX, CY = 202.0, 202.0, 159.93827, 119.938015


def median_us(launch, refresh, n=25, warm=5):
    ts = []
    for i in range(warm + n):
        refresh()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def window_sizes(params, B, H, W, inverse):
    """Candidate-window sizes of the adjoints, restated on the host in float64 from the device record (the bounding box of the 2x2-pixel
    support mapped into output space, widened as the kernel widens it)."""
    import numpy as np
    p = params.double().cpu().numpy()
    out = []
    ys, xs = np.mgrid[0:H, 0:W]
    for b in range(B):
        r = p[b]
        lo = [np.full((H, W), np.inf), np.full((H, W), np.inf)]
        hi = [np.full((H, W), -np.inf), np.full((H, W), -np.inf)]
        for k in range(4):
            ix, iy = xs + (1.0 if k & 1 else -1.0), ys + (1.0 if k & 2 else -1.0)
            u = ((2 * ix + 1) / W - 1) * (W / 2) + CX
            v = ((2 * iy + 1) / H - 1) * (H / 2) + CY
            if inverse:
                s, t = u / r[29] + r[27], v / r[30] + r[28]
                d = r[24] * s + r[25] * t + r[26]
                q = ((r[18] * s + r[19] * t + r[20]) / d, (r[21] * s + r[22] * t + r[23]) / d)
            else:
                d = r[6] * u + r[7] * v + r[8]
                q = (r[29] * ((r[0] * u + r[1] * v + r[2]) / d - r[27]), r[30] * ((r[3] * u + r[4] * v + r[5]) / d - r[28]))
            for a in (0, 1):
                lo[a], hi[a] = np.minimum(lo[a], q[a]), np.maximum(hi[a], q[a])
        n = 1
        for a, N in ((0, W), (1, H)):
            m = 0.125 + (hi[a] - lo[a]) / 64
            n0, n1 = np.clip(np.floor(lo[a] - m), 0, N), np.clip(np.ceil(hi[a] + m), -1, N - 1)
            n = n * np.maximum(n1 - n0 + 1, 0)
        out.append(n)
    n = np.stack(out)
    return float(n.mean()), int(n.max())


def main():
    lib, H, W = L.lib(), 240, 320
    print("%-46s %5s %10s %10s %7s %9s" % ("kernel", "batch", "fwd us", "bwd us", "bwd/fwd", "bwd GB/s"))
    for B in (1, 32):
        b = S.synthetic_batch(B, H, W, 1234)
        wp = Warping2DOFAlignment(FX, FY, CX, CY, device="cuda")
        params = wp._params(b["gravity"].cuda(), b["aligned_direction"].cuda())
        master = b["image"].cuda().float().contiguous()
        gmaster = S.normal01(5, "bench.dy", (B, 3, H, W)).float().cuda()
        x, dy, out = torch.empty_like(master), torch.empty_like(master), torch.empty_like(master)
        refresh = lambda: (x.copy_(master), dy.copy_(gmaster))
        st = L.current_stream
        nbytes = 2 * master.numel() * 4
        cases = [
            ("warp2dof_fwd", lambda: lib.vidc_warp2dof_fwd(L.ptr(x), L.ptr(params), L.ptr(out), B, 3, H, W, CX, CY, 0, st()),
             lambda: lib.vidc_warp2dof_fwd_backward(L.ptr(dy), L.ptr(params), L.ptr(out), B, 3, H, W, CX, CY, 0, st()), nbytes, False),
            ("warp2dof_inv_rot_norm (normalize)", lambda: lib.vidc_warp2dof_inv_rot_norm(L.ptr(x), L.ptr(params), L.ptr(out), B, H, W, CX, CY, 0, 1, st()),
             lambda: lib.vidc_warp2dof_inv_rot_norm_backward(L.ptr(x), L.ptr(dy), L.ptr(params), L.ptr(out), B, H, W, CX, CY, 0, 1, st()),
             3 * master.numel() * 4, True),
        ]
        for name, fwd, bwd, nb, inverse in cases:
            tf, tb = median_us(fwd, refresh), median_us(bwd, refresh)
            mean_w, max_w = window_sizes(params, B, H, W, inverse)
            print("%-46s %5d %10.1f %10.1f %7.2f %9.1f   window: mean %.1f max %d candidates" % (name, B, tf, tb, tb / tf, nb / tb * 1e-3, mean_w, max_w))
    B, h, w, Cc = 8, 15, 20, 1024
    ym = S.normal01(5, "bench.y", (B, h, w, Cc)).float().cuda().relu()
    gm = S.normal01(5, "bench.g", (B, h, w, Cc)).float().cuda()
    y, g, dc = torch.empty_like(ym), torch.empty_like(gm), torch.empty_like(ym)
    scale, shift = (0.5 + S.uniform01(5, "bench.s", (Cc,)).float()).cuda(), (0.1 * S.normal01(5, "bench.b", (Cc,)).float()).cuda()
    ds, db = torch.empty_like(scale), torch.empty_like(shift)
    M = B * h * w
    sc = torch.empty(lib.vidc_train_scratch_bytes(M, Cc) + 256, dtype=torch.uint8, device="cuda")
    refresh = lambda: (y.copy_(ym), g.copy_(gm))
    tf = median_us(lambda: lib.vidc_relu_backward(L.ptr(g), L.ptr(y), L.ptr(dc), M, Cc, Cc, Cc, Cc, 0, L.current_stream()), refresh)
    tb = median_us(lambda: lib.vidc_affine_act_backward(L.ptr(g), L.ptr(y), None, L.ptr(scale), L.ptr(shift), L.ptr(dc), L.ptr(ds), L.ptr(db), M, Cc, Cc, Cc, Cc, Cc,
                                                        1, L.ptr(sc), L.current_stream()), refresh)
    print("%-46s %5d %10.1f %10.1f %7.2f %9.1f   (yardstick: vidc_relu_backward over the same rows)"
          % ("affine_act_backward 15x20x1024", B, tf, tb, tb / tf, 3 * ym.numel() * 4 / tb * 1e-3))


if __name__ == "__main__":
    main()
