"""Drop-in for the reference's `Warping2DOFAlignment` (networks/warping_2dof_alignment.py:5-24, 108-310):
same constructor and method signatures, but each method is two HIP launches (per-sample geometry + fused
gather) through libvidc.so instead of ~520 ATen calls.  No weights; not an nn.Module (like the reference).

`warp_normal_image_with_gravity_center_aligned` is read as its sibling `warp_with_gravity_center_aligned` reads: as shipped (:259-260) the
reference's method fails on its first line -- it unpacks two of `_build_homography`'s three values and inverts Cg_H_C with torch.inverse
where the sibling takes the third, K R^T K^-1.  `warp_with_homography` builds its geometry record on the host (one launch).
"""
import math

import numpy as np
import torch

from .. import _lib as L
from .. import ops


class Warping2DOFAlignment:
    def __init__(self, fx=577.87061 * 0.5, fy=577.87061 * 0.5, cx=319.87654 * 0.5, cy=239.87603 * 0.5,
                 align_corners=False, device="cuda"):
        self.device = torch.device(device)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.W, self.H = int(math.ceil(2 * cx)), int(math.ceil(2 * cy))
        k = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
        self.K_host = k.astype(np.float32)
        self.K_inv_host = np.linalg.inv(k).astype(np.float32)       # fp64 inverse cast to fp32, as the reference does
        # grid_sample convention: False = what torch >= 1.3 does when the reference omits the argument (the oracle's
        # behaviour); True = the torch-1.2 behaviour the checkpoints were trained with.
        self.align_corners = bool(align_corners)
        self._kinv_dev = {}

    def kinv(self, device):
        key = str(device)
        if key not in self._kinv_dev:
            self._kinv_dev[key] = torch.from_numpy(self.K_inv_host.reshape(-1).copy()).to(device)
        return self._kinv_dev[key]

    def _params(self, I_g, I_a):
        B = I_g.shape[0]
        g = I_g.reshape(B, 3).contiguous().float()
        a = I_a.reshape(B, 3).contiguous().float()
        p = torch.empty((B, L.WARP_PARAMS), dtype=torch.float32, device=g.device)
        L.check(L.lib().vidc_warp2dof_params(L.ptr(g), L.ptr(a), B, self.fx, self.fy, self.cx, self.cy,
                                             L.ptr(self.kinv(g.device)), self.W, self.H, L.ptr(p), L.current_stream()),
                "warp2dof_params")
        return p

    @staticmethod
    def _require_device(x):
        if not x.is_cuda:
            raise RuntimeError("Warping2DOFAlignment runs on the GPU only (HIP path, no CPU fallback)")

    @staticmethod
    def _mode(interp_mode):
        """F.grid_sample's `mode` string -> VIDC_WARP_*."""
        if interp_mode not in ops.WARP_MODES:
            raise ValueError("interp_mode must be 'bilinear', 'nearest' or 'bicubic', got %r" % (interp_mode,))
        return ops.WARP_MODES[interp_mode]

    def _prepare(self, x, I_g, I_a, channels=None):
        """What every gravity warp of an image starts with: the device and shape checks, then (the geometry record, the Cg_H_C it returns).
        x is (B,C,H,W), or (B,H,W) with channels=None only: the channel check reads x.shape[1]."""
        self._require_device(x)
        assert x.shape[0] == I_g.shape[0] and (channels is None or x.shape[1] == channels)
        assert tuple(x.shape[-2:]) == (self.H, self.W), "image must be %dx%d" % (self.H, self.W)
        p = self._params(I_g, I_a)
        return p, p[:, 0:9].reshape(x.shape[0], 3, 3).clone()

    def warp_with_gravity_center_aligned(self, x, I_g, I_a, interp_mode="bilinear"):
        mode = self._mode(interp_mode)
        p, Cg_H_C = self._prepare(x, I_g, I_a)
        squeeze = x.dim() == 3
        if squeeze:
            x = x.view(x.shape[0], 1, x.shape[1], x.shape[2])
        x = x.contiguous().float()
        B, Cc = x.shape[0], x.shape[1]
        if mode == 0:
            y = torch.empty_like(x)
            L.check(L.lib().vidc_warp2dof_fwd(L.ptr(x), L.ptr(p), L.ptr(y), B, Cc, self.H, self.W, self.cx, self.cy,
                                              int(self.align_corners), L.current_stream()), "warp2dof_fwd")
        else:
            y = ops.warp2dof_fwd_mode(x, p, self.cx, self.cy, self.align_corners, mode)
        return (Cg_H_C, y.view(B, self.H, self.W)) if squeeze else (Cg_H_C, y)

    def inverse_warp_normal_image_with_gravity_center_aligned(self, x, I_g, I_a, normalize=False):
        p, Cg_H_C = self._prepare(x, I_g, I_a, channels=3)
        x = x.contiguous().float()
        z = torch.empty_like(x)
        L.check(L.lib().vidc_warp2dof_inv_rot_norm(L.ptr(x), L.ptr(p), L.ptr(z), x.shape[0], self.H, self.W, self.cx, self.cy,
                                                   int(self.align_corners), int(normalize), L.current_stream()),
                "warp2dof_inv_rot_norm")
        return Cg_H_C, z

    def warp_normal_image_with_gravity_center_aligned(self, x, I_g, I_a, interp_mode="bilinear"):
        """The forward companion of the inverse normal warp (:258-290): the gather of warp_with_gravity_center_aligned, then z = Cg_R_C y."""
        mode = self._mode(interp_mode)
        p, Cg_H_C = self._prepare(x, I_g, I_a, channels=3)
        return Cg_H_C, ops.warp2dof_fwd_mode(x, p, self.cx, self.cy, self.align_corners, mode, rotate=True)

    def image_sampler_forward_inverse(self, I_g, I_a):
        """(C_R_Cg_ret, grid_sampler, inv_grid_sampler) (:158-214): the sampling grids of the two warps as F.grid_sample takes them, and
        Cg_R_C^T; a sample tilted so far that its corner box leaves [0.8, 2.2] in w_max / h_max gets identity grids and I3 (:178-187)."""
        self._require_device(I_g)
        return ops.warp2dof_grids(self._params(I_g, I_a), self.H, self.W, self.cx, self.cy)

    def homography_record(self, Cg_H_C):
        """The 32-float record of vidc_warp2dof_params for a GIVEN homography (warp_with_homography, :292-310), on the host in float64 as the
        reference computes it, cast to fp32: R = I, numpy's inverse, the corner box and kw = W / (w_max - w_min), kh = H / (h_max - h_min)
        -- independent scales, no 4:3 rule."""
        Hm = np.asarray(Cg_H_C.detach().cpu() if torch.is_tensor(Cg_H_C) else Cg_H_C, dtype=np.float64).reshape(3, 3)
        corners = np.array([[0, 0, 1], [self.W - 1, 0, 1], [0, self.H - 1, 1], [self.W - 1, self.H - 1, 1]], dtype=np.float64).T
        c = Hm @ corners
        c = c / c[2, :]
        h_min, h_max, w_min, w_max = c[1].min(), c[1].max(), c[0].min(), c[0].max()
        rec = np.zeros(L.WARP_PARAMS, dtype=np.float64)
        rec[0:9], rec[9:18], rec[18:27] = Hm.reshape(-1), np.identity(3).reshape(-1), np.linalg.inv(Hm).reshape(-1)
        rec[27:31] = w_min, h_min, self.W / (w_max - w_min), self.H / (h_max - h_min)
        return rec.astype(np.float32)

    def warp_with_homography(self, x, Cg_H_C):
        if x.dim() != 4 or x.shape[0] != 1:
            raise RuntimeError("warp_with_homography takes one image (1,C,H,W), as the reference's single grid does; got %s" % (tuple(x.shape),))
        self._require_device(x)
        assert tuple(x.shape[-2:]) == (self.H, self.W), "image must be %dx%d" % (self.H, self.W)
        p = torch.from_numpy(self.homography_record(Cg_H_C)).view(1, L.WARP_PARAMS).to(x.device)
        return Cg_H_C, ops.warp2dof_fwd_mode(x, p, self.cx, self.cy, self.align_corners, 0)
