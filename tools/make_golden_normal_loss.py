#!/usr/bin/env python3
"""Record of the reference's normal loss for tests/test_sn_training.py (build container only: it imports the reference's normal_utils.py,
found where oracle/tools/ref_shims.py says the reference lives; nothing of the reference's text is copied).

    python tools/make_golden_normal_loss.py [out_dir]      ->  tests/golden/normal_loss.npz

Inputs (2, 3, 12, 16), seeded: `pred` of length 0.5..0.95 in random directions, a raw `normal_gt` of non-unit length, a mask of about
70 %.  Stored with them, for the two values of `normalize_prediction`, what `_network_loss` computes from them (network_run.py:182-189:
the ground truth through F.normalize, the mask as `> 0`) with compute_normal_vectors_loss_l1: the loss, the angle sum, and torch's
autograd gradient of the loss with respect to `pred`.
  *_raw:  normalize_prediction=False, the reference's code as shipped.
  *_norm: normalize_prediction=True.  That branch calls `Normalize`, a name normal_utils.py never defines; the one missing name is injected
          into the imported module as F.normalize(x, dim=1) -- the function the network's own last line uses -- and nothing else is changed.
The inputs are drawn again (next seed) until no unmasked pixel has |n . gh| > 0.999 (acos is ill-conditioned there, and the record is
fp32) and no element has |n_c - gh_c| < 1e-6 (a sign tie in the L1 gradient), for both readings of n."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_shims  # noqa: E402

sys.path.insert(0, ref_shims.REFERENCE_ROOT)
import normal_utils  # noqa: E402  (the reference's)

SHAPE = (2, 3, 12, 16)


def draw(seed):
    g = torch.Generator().manual_seed(seed)
    B, _, H, W = SHAPE
    direction = F.normalize(torch.randn(SHAPE, generator=g), dim=1)
    pred = direction * (0.5 + 0.45 * torch.rand(B, 1, H, W, generator=g))
    normal_gt = torch.randn(SHAPE, generator=g) * (0.5 + 2.0 * torch.rand(B, 1, H, W, generator=g))
    mask = (torch.rand(B, H, W, generator=g) < 0.7).float()
    return pred, normal_gt, mask


def well_conditioned(pred, normal_gt, mask):
    gh = F.normalize(normal_gt.double(), dim=1)
    on = mask[:, None] > 0
    for n in (pred.double(), F.normalize(pred.double(), dim=1)):
        if ((n * gh).sum(1, keepdim=True).abs()[on] > 0.999).any() or ((n - gh).abs()[on.expand_as(n)] < 1e-6).any():
            return False
    return True


def reference_loss(pred, normal_gt, mask, normalize_prediction):
    p = pred.clone().requires_grad_(True)
    with torch.enable_grad():
        loss, angle = normal_utils.compute_normal_vectors_loss_l1(F.normalize(normal_gt), p, (mask > 0)[:, None, :, :], normalize_prediction)
        loss.backward()
    return np.float32(loss.item()), np.float32(angle.item()), p.grad.numpy().copy()


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    seed = 1234
    while not well_conditioned(*draw(seed)):
        seed += 1
    pred, normal_gt, mask = draw(seed)
    assert well_conditioned(pred, normal_gt, mask)
    rec = {"seed": np.int64(seed), "pred": pred.numpy(), "normal_gt": normal_gt.numpy(), "mask": mask.numpy()}
    rec["loss_raw"], rec["angle_raw"], rec["dpred_raw"] = reference_loss(pred, normal_gt, mask, False)
    assert not hasattr(normal_utils, "Normalize"), "the reference defines Normalize now: record its own reading instead"
    normal_utils.Normalize = lambda x: F.normalize(x, dim=1)
    rec["loss_norm"], rec["angle_norm"], rec["dpred_norm"] = reference_loss(pred, normal_gt, mask, True)
    path = os.path.join(out_dir, "normal_loss.npz")
    np.savez_compressed(path, **rec)
    print("%s: seed %d, N = %d, loss %.6f / %.6f, angle %.3f / %.3f, %d bytes" % (path, seed, int(mask.sum()), rec["loss_raw"], rec["loss_norm"], rec["angle_raw"],
                                                                                  rec["angle_norm"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
