"""Times the small-map 3x3 layers as Winograd F(4x4) in ONE launch (csrc/wfused.hip) against the three-launch path (input transform + grouped GEMM on the
table's tile + output transform), weights HBM-cold (a rotation of weight copies), back-to-back launches between two HIP events.

    python tools/wfused_bench.py [--iters 40] [--only stem]

For the 64-channel stem layers the fused launch is timed in both forms of the tile: the persistent Cin = 64 form the launcher picks for them, and the
16 tiles x 32 channels form of the small maps (VIDC_WFUSED_STEM_MIN_TILES=0), the baseline the Cin = 64 form was built against.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from vi_depth_completion_amd import _lib as L
from vi_depth_completion_amd import ops

torch.set_grad_enabled(False)
DEV = "cuda"
# (B, H, W, cin, cout, G, label, tile of the three-launch GEMM in the measured table)
SHAPES = [(4, 16, 20, 256, 256, 4, "layer3 conv2 x22", 28), (4, 32, 40, 128, 128, 4, "layer2 conv2 x3", 29), (4, 16, 20, 512, 512, 2, "sn/feature3_upsamping.3", 28),
          (4, 32, 40, 256, 256, 3, "sn/feature2_upsamping.3", 29), (4, 16, 20, 256, 256, 1, "layer3, one group (head tick)", 28), (4, 16, 20, 256, 256, 3, "layer3, three groups (tail tick)", 28),
          (4, 128, 160, 64, 64, 4, "stem conv1_2", 29), (4, 128, 160, 64, 128, 4, "stem conv1_3", 1),
          (4, 128, 160, 64, 64, 1, "stem conv1_2, one group (head tick)", 29), (4, 128, 160, 64, 128, 3, "stem conv1_3, three groups (tail tick)", 1)]


def timed(fn, iters):
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i + 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--only", default="", help="time only the shapes whose label contains this")
    a = ap.parse_args()
    for (B, H, W, cin, cout, G, label, tile) in SHAPES:
        if a.only not in label:
            continue
        x = torch.randn(B, H, W, G * cin, device=DEV)
        copies = max(2, min(16, (1 << 29) // (G * 36 * cout * cin * 4)))
        us = [torch.randn(G * 36, cout, cin, device=DEV) * 0.05 for _ in range(copies)]      # (random values: the fused launch reads them in its packed order, the GEMM as [pos][Cout][Cin])
        s1, b1 = torch.rand(G, cout, device=DEV) + 0.5, torch.randn(G, cout, device=DEV) * 0.1
        t_f = timed(lambda i: ops.conv3x3_winograd_fused(x, None, s1, b1, relu1=True, u=us[i % copies]), a.iters)
        t_f4 = None
        if cin == 64 and cout % 64 == 0 and "VIDC_WFUSED_STEM_MIN_TILES" not in os.environ:
            os.environ["VIDC_WFUSED_STEM_MIN_TILES"] = "0"          # (the launcher reads it at every launch)
            t_f4 = timed(lambda i: ops.conv3x3_winograd_fused(x, None, s1, b1, relu1=True, u=us[i % copies]), a.iters)
            del os.environ["VIDC_WFUSED_STEM_MIN_TILES"]
        # the three launches separately (the python wrappers allocate; time each kernel family on its own)
        v = ops.winograd_input_transform(x, cin, 4)
        t_in = timed(lambda i: ops.winograd_input_transform(x, cin, 4), a.iters)
        tiles = v.shape[0]
        one, zero = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
        t_g = timed(lambda i: ops.conv2d_bn_act(v.view(1, 1, tiles, -1), us[i % copies].view(G * 36, cout, cin), one, zero, 1, 1, tile=tile, groups=G * 36), a.iters)
        mm = torch.randn(tiles, 36 * G * cout, device=DEV)
        t_out = timed(lambda i: ops.winograd_output_transform(mm, B, H, W, cout, 4, s1, b1, relu1=True), a.iters)
        flop = 2.0 * tiles * 36 * cin * cout * G
        print("%-34s B%d %dx%d %d->%d G%d  %5.2f GFLOP | fused %6.1f us (%5.1f TF)%s | three launches %5.1f + %5.1f + %5.1f = %6.1f us" %
              (label, B, H, W, cin, cout, G, flop / 1e9, t_f, flop / t_f / 1e6, "" if t_f4 is None else " [small-map form %6.1f us]" % t_f4,
               t_in, t_g, t_out, t_in + t_g + t_out), flush=True)


if __name__ == "__main__":
    main()
