"""Device-side frame pre-processing: the per-frame work of the reference's `DemoDataset.__getitem__` (dataset.py:461-520) behind the
same output dictionary, so a camera stream can be fed to `DepthCompletionPipeline` without a PIL/Python DataLoader per frame.

    pre = FramePreprocessor(device)                       # tables for 640x480 -> 320x240, DemoDataset's intrinsics
    batch = pre(image_u8, gravity_raw, klt_tracks)        # image_u8: (B,480,640,3) uint8; gravity_raw: (B,3); klt_tracks: list of (N_i,4)
    depth = pipeline._call_cnn(batch)

What runs where: the resize (+ToTensor) and the sparse-point rasterisation are HIP kernels (csrc/preprocess.hip, bit-identical to
Pillow / to the reference's float64 loop); the gravity sign flip and alignment rule are three floats per frame and stay on the host
in the reference's own torch-CPU arithmetic (dataset.py:472-483); the homogeneous grid is a constant (dataset.py:34-42).
There is no CPU fallback for the kernels."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

DEMO_FC = (202.9953, 202.9540)       # dataset.py:456-457: "compensates for both cropping and scaling"
DEMO_CC = (159.7645, 122.0951)


def resize_tables(in_size, out_size):
    """(bounds int32 [out,2], coeffs int32 [out,ksize]) of Pillow's bilinear resample for one axis (host computation in libvidc)."""
    lib = L.lib()
    ks = C.c_int(0)
    L.check(lib.vidc_resize_coeffs(in_size, out_size, None, None, 0, C.byref(ks)), "resize_coeffs")
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ks.value), np.int32)
    L.check(lib.vidc_resize_coeffs(in_size, out_size, bounds.ctypes.data, coeffs.ctypes.data, coeffs.size, C.byref(ks)), "resize_coeffs")
    return bounds, coeffs


def nearest_table(in_size, out_size):
    """int32 [out]: source index of every output coordinate of Pillow's NEAREST resize along one axis (host computation in libvidc)."""
    t = np.zeros(out_size, np.int32)
    L.check(L.lib().vidc_nearest_table(in_size, out_size, t.ctypes.data), "nearest_table")
    return t


def gravity_and_alignment(gravity_raw):
    """dataset.py:472-483, host, torch CPU fp32 like the reference."""
    g = torch.tensor(np.asarray(gravity_raw, dtype=np.float64), dtype=torch.float)
    g[1] = -g[1]
    g[2] = -g[2]
    psi = g[1] * g[1] + g[2] * g[2]
    if psi < 1e-4:
        a = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float)
    else:
        pitch = torch.atan2(g[2], g[1])
        if torch.cos(pitch) > 0.707:
            a = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float)
        else:
            a = torch.tensor([0.0, torch.cos(pitch), torch.sin(pitch)], dtype=torch.float)
    return g, a


def homogeneous_coordinates(fc, cc, W, H):
    """dataset.py:34-42 (float64 numpy, then float32)."""
    hom = np.zeros((H, W, 3))
    hom[:, :, 2] = 1
    xx, yy = np.meshgrid(np.arange(W), np.arange(H))
    hom[:, :, 0] = (xx - cc[0]) / fc[0]
    hom[:, :, 1] = (yy - cc[1]) / fc[1]
    return torch.from_numpy(hom.astype(np.float32))


class FramePreprocessor:
    def __init__(self, device="cuda", in_hw=(480, 640), out_hw=(240, 320), fc=DEMO_FC, cc=DEMO_CC):
        if not torch.cuda.is_available():
            raise RuntimeError("FramePreprocessor needs a GPU: the HIP path has no CPU fallback")
        self.device = torch.device(device)
        self.in_hw, self.out_hw, self.fc, self.cc = tuple(in_hw), tuple(out_hw), tuple(fc), tuple(cc)
        bx, kx = resize_tables(in_hw[1], out_hw[1])
        by, ky = resize_tables(in_hw[0], out_hw[0])
        self.ksx, self.ksy = kx.shape[1], ky.shape[1]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.bx, self.kx, self.by, self.ky = up(bx), up(kx), up(by), up(ky)
        self.homogeneous = homogeneous_coordinates(fc, cc, out_hw[1], out_hw[0]).to(self.device)
        self.nx, self.ny = up(nearest_table(in_hw[1], out_hw[1])), up(nearest_table(in_hw[0], out_hw[0]))

    def resize(self, image_u8):
        """(B,H,W,C) uint8 on the device -> (B,C,Ho,Wo) float32 = ToTensor(PIL bilinear resize)."""
        if not image_u8.is_cuda or image_u8.dtype != torch.uint8:
            raise RuntimeError("resize() takes a uint8 GPU tensor (B,H,W,C)")
        x = image_u8.contiguous()
        B, H, W, Cc = x.shape
        assert (H, W) == self.in_hw, "tables were built for %s input, got %s" % (self.in_hw, (H, W))
        Ho, Wo = self.out_hw
        y = torch.empty((B, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
        L.check(L.lib().vidc_resize_bilinear_u8_to_chw(L.ptr(x), L.ptr(y), B, H, W, Cc, Ho, Wo, L.ptr(self.bx), L.ptr(self.kx), self.ksx,
                                                       L.ptr(self.by), L.ptr(self.ky), self.ksy, L.current_stream()), "resize")
        return y

    def gt_depth(self, depth_u16, millimetres_per_metre=1000.0):
        """(B,H,W) uint16 millimetre depth maps on the device -> (B,1,Ho,Wo) float32 metres: the ground truth of the training and
        evaluation streams, `Image.open(d).convert('F').resize((320, 240), resample=Image.NEAREST)` then `/ 1000.0`
        (dataset.py:283-286), bit for bit -- `sample['depth']` of network_run.py:165-172, 216-225 without a PIL pass per frame."""
        if not depth_u16.is_cuda or depth_u16.dtype not in (torch.uint16, torch.int16):
            raise RuntimeError("gt_depth() takes a uint16 GPU tensor (B,H,W) (a 16-bit depth PNG as the camera driver delivers it)")
        x = depth_u16.contiguous()
        B, H, W = x.shape
        assert (H, W) == self.in_hw, "tables were built for %s input, got %s" % (self.in_hw, (H, W))
        Ho, Wo = self.out_hw
        y = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=x.device)
        L.check(L.lib().vidc_resize_nearest_u16_depth(L.ptr(x), L.ptr(y), B, H, W, Ho, Wo, L.ptr(self.nx), L.ptr(self.ny), float(millimetres_per_metre),
                                                      L.current_stream()), "gt_depth")
        return y

    def _upload(self, t):
        """Small host tensor -> fresh device tensor through (cached) pinned memory: a copy out of pageable memory would block the host
        until the device has caught up with everything queued before it -- a whole tick of the stream being pre-processed for."""
        p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        p.copy_(t)
        return p.to(self.device, non_blocking=True)

    def rasterize(self, klt_tracks):
        """list of B arrays (N_i, 4) = (id, X, Y, Z) -> (B,1,Ho,Wo) float32 sparse depth."""
        B = len(klt_tracks)
        Ho, Wo = self.out_hw
        rows = [np.atleast_2d(np.asarray(t, dtype=np.float64)).reshape(-1, 4) if np.size(t) else np.zeros((0, 4)) for t in klt_tracks]
        offs = np.zeros(B + 1, np.int32)
        offs[1:] = np.cumsum([r.shape[0] for r in rows])
        allr = np.concatenate(rows) if offs[-1] else np.zeros((1, 4))
        tr = self._upload(torch.from_numpy(np.ascontiguousarray(allr)))
        of = self._upload(torch.from_numpy(offs))
        d = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=self.device)
        L.check(L.lib().vidc_rasterize_sparse_depth(L.ptr(tr), L.ptr(of), B, self.fc[0], self.fc[1], self.cc[0], self.cc[1], L.ptr(d), Ho, Wo,
                                                    L.current_stream()), "rasterize")
        self._keep = (tr, of)
        return d

    def __call__(self, image_u8, gravity_raw, klt_tracks, depth_u16=None):
        """The collated batch dictionary of DemoDataset (dataset.py:515-520), on the device; with `depth_u16` also the 'depth' entry of
        the Azure / ScanNet loaders (dataset.py:283-286, 349)."""
        img = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.ascontiguousarray(image_u8))
        img = img.to(self.device, non_blocking=True)
        B = img.shape[0]
        ga = [gravity_and_alignment(g) for g in np.asarray(gravity_raw, dtype=np.float64).reshape(B, 3)]
        out = {"image": self.resize(img), "sparse_depth": self.rasterize(klt_tracks),
               "gravity": self._upload(torch.stack([g for g, _ in ga])), "aligned_direction": self._upload(torch.stack([a for _, a in ga])),
               "homogeneous_coordinates": self.homogeneous.unsqueeze(0).expand(B, -1, -1, -1)}
        if depth_u16 is not None:
            d16 = depth_u16 if torch.is_tensor(depth_u16) else torch.from_numpy(np.ascontiguousarray(depth_u16))
            out["depth"] = self.gt_depth(d16.to(self.device, non_blocking=True))
        return out


# ---- training batches: ScanNetSmallFramesDataset (dataset.py:58-250) and NYUDataset (dataset.py:355-441) ---------------------------
SCANNET_FC = (577.87061 / 2, 580.25851 / 2)      # dataset.py:91-92
SCANNET_CC = (319.87654 / 2, 239.87603 / 2)
TRACK_DIVISOR = 2.0                              # both loaders: "the tracks have been created for 640x480 image" (dataset.py:204, 416-417)


def scannet_gravity_and_alignment(gravity):
    """dataset.py:132 and compute_alignment_tensor (dataset.py:45-55), host, torch CPU fp32 like the reference: no sign flip."""
    g = torch.tensor(np.asarray(gravity, dtype=np.float64), dtype=torch.float)
    psi = g[1] * g[1] + g[2] * g[2]
    if psi < 1e-6:
        return g, g
    pitch = torch.atan2(g[2], g[1])
    if torch.cos(pitch) > 0.3:
        return g, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float)
    return g, g


def track_rows(klt_tracks):
    """list of B track tables -> (rows float64 [N,4] of all images, offsets int32 [B+1]).  A table without rows (an empty file, a failed
    read) contributes none; the three-column table of tracked KLT features (id, x, y: dataset.py:177, 189) gets a zero depth column."""
    rows = []
    for t in klt_tracks:
        a = np.atleast_2d(np.asarray(t, dtype=np.float64))
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((a.shape[0], 1))], axis=1)
        rows.append(a if a.shape[1] == 4 else np.zeros((0, 4)))
    offs = np.zeros(len(rows) + 1, np.int32)
    offs[1:] = np.cumsum([r.shape[0] for r in rows])
    return (np.concatenate(rows) if offs[-1] else np.zeros((0, 4))), offs


def draw_sparse_sample(counts, num_points, rng=np.random):
    """The draws of dataset.py:193-200 for one batch, image by image: `counts[b]` non-zero ground-truth pixels, `num_points[b]` rows in
    the track table.  num_points >= count: the clone, nothing is drawn (nsel -1).  Otherwise permutation(count)[0:num_points] -- drawn
    even for num_points == 0 -- natively on the MT19937 state when `rng` is numpy's legacy generator (plane._LegacyStream; committed
    once), through rng.permutation otherwise.  Returns (perm int32 of all images, sel_off int32 [B], nsel int32 [B])."""
    from .plane import _LegacyStream
    stream = _LegacyStream.open(rng)
    perm, sel_off, nsel, off = [], [], [], 0
    for count, n in zip(counts, num_points):
        count, n = int(count), int(n)
        sel_off.append(off)
        if n >= count:
            nsel.append(-1)
            continue
        p = stream.permutation_prefix(count, n) if stream is not None else np.asarray(rng.permutation(count)[0:n], dtype=np.int32)
        perm.append(p)
        nsel.append(n)
        off += n
    if stream is not None:
        stream.commit()
    return (np.concatenate(perm).astype(np.int32) if perm else np.zeros(0, np.int32)), np.asarray(sel_off, np.int32), np.asarray(nsel, np.int32)


class _TrainingBatches(FramePreprocessor):
    """What the two training-batch classes share: input checks, the byte-image decode and the pixel-track map (csrc/train_preprocess.hip)."""

    def _input(self, x, name, dtypes, shape):
        """A raw array of the caller's: numpy -> uploaded through pinned memory; a torch tensor has to be on the GPU already."""
        if isinstance(x, np.ndarray):
            if x.dtype == np.uint16:
                x = x.view(np.int16)
            x = self._upload(torch.from_numpy(np.ascontiguousarray(x)))
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError("%s: a numpy array or a GPU tensor is needed (there is no CPU path)" % name)
        if x.dtype not in dtypes:
            raise RuntimeError("%s: dtype %s, expected %s" % (name, x.dtype, " or ".join(str(d) for d in dtypes)))
        if tuple(x.shape) != tuple(shape):
            raise RuntimeError("%s: shape %s, expected %s" % (name, tuple(x.shape), tuple(shape)))
        return x.contiguous()

    def decode(self, u8, mode):
        """(B,H,W,C) or (B,H,W) uint8 on the device -> (B,C,H,W) float32 by one of the reference's byte expressions (_lib.U8_*)."""
        if not torch.is_tensor(u8) or not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() not in (3, 4):
            raise RuntimeError("decode() takes a uint8 GPU tensor (B,H,W,C) or (B,H,W)")
        x = u8.contiguous()
        B, H, W = x.shape[:3]
        Cc = x.shape[3] if x.dim() == 4 else 1
        y = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
        L.check(L.lib().vidc_u8_decode_chw(L.ptr(x), L.ptr(y), B, H, W, Cc, mode, L.current_stream()), "u8_decode_chw")
        return y

    def pixel_tracks(self, klt_tracks, gt_depth=None):
        """list of B tables (N_i,4) = (id, x, y, d) in 640x480 pixel coordinates -> (B,1,Ho,Wo) float32 sparse depth; with `gt_depth`
        (B,1,Ho,Wo) the ground truth at the tracks' pixels instead of d."""
        B = len(klt_tracks)
        Ho, Wo = self.out_hw
        allr, offs = track_rows(klt_tracks)
        n = int(offs[-1])
        tr = self._upload(torch.from_numpy(np.ascontiguousarray(allr))) if n else None
        of = self._upload(torch.from_numpy(offs))
        d = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=self.device)
        lib = L.lib()
        scratch = torch.empty(lib.vidc_rasterize_pixel_tracks_scratch_bytes(B, Ho, Wo), dtype=torch.uint8, device=self.device)
        L.check(lib.vidc_rasterize_pixel_tracks(L.ptr(tr), L.ptr(of), n, B, TRACK_DIVISOR, L.ptr(gt_depth), L.ptr(d), Ho, Wo, L.ptr(scratch),
                                                L.current_stream()), "rasterize_pixel_tracks")
        self._keep = (tr, of, scratch)
        return d


class ScanNetFramePreprocessor(_TrainingBatches):
    """The batch dictionary of ScanNetSmallFramesDataset (dataset.py:95-247) on the device, restricted to the keys main.py:262-280 and
    network_run.py:150-225 read: image, depth, mask, normal, sparse_depth, gravity, aligned_direction, homogeneous_coordinates and
    predicted_normal.  File reading and the PNG decode stay with the caller, who hands over the raw arrays:

        pre = ScanNetFramePreprocessor(device)
        batch = pre(color_u8, depth_u16, orient_u8, mask_u8, gravity, klt_tracks)      # (B,240,320,3) / (B,240,320) / (B,3) / list of (N_i,4)

    With generate_random_sparse_pointcloud the sample of dataset.py:193-202 needs the number of non-zero ground-truth pixels of every image
    on the host before it can draw: ONE device->host read of B counts per batch (the reference's torch.nonzero is the same point of
    synchronisation), then the draws in batch order from `rng`."""

    def __init__(self, device="cuda", hw=(240, 320), read_depths_from_pointcloud=True, generate_random_sparse_pointcloud=False, rng=np.random):
        super().__init__(device, in_hw=hw, out_hw=hw, fc=SCANNET_FC, cc=SCANNET_CC)
        self.read_pointcloud, self.random_sparse, self.rng = bool(read_depths_from_pointcloud), bool(generate_random_sparse_pointcloud), rng
        self._count_pinned = self._count_event = None

    def random_sparse_sample(self, depth, klt_tracks):
        """dataset.py:192-202 for a batch: depth (B,1,H,W) float32 on the device -> (B,1,H,W) sparse depth."""
        lib, st = L.lib(), L.current_stream()
        B, HW = depth.shape[0], depth.shape[2] * depth.shape[3]
        count = torch.empty(B, dtype=torch.int32, device=self.device)
        index = torch.empty((B, HW), dtype=torch.int32, device=self.device)
        scratch = torch.empty(lib.vidc_nonzero_compact_scratch_bytes(B, HW), dtype=torch.uint8, device=self.device)
        L.check(lib.vidc_nonzero_compact(L.ptr(depth), B, HW, L.ptr(count), L.ptr(index), L.ptr(scratch), st), "nonzero_compact")
        if self._count_pinned is None or self._count_pinned.numel() != B:
            self._count_pinned = torch.empty(B, dtype=torch.int32, pin_memory=True)
            self._count_event = torch.cuda.Event()
        self._count_pinned.copy_(count, non_blocking=True)
        self._count_event.record()
        num_points = [np.atleast_2d(np.asarray(t)).shape[0] for t in klt_tracks]      # dataset.py:183, 193: an empty file counts 1, a failed read 0
        self._count_event.synchronize()
        perm, sel_off, nsel = draw_sparse_sample(self._count_pinned.numpy(), num_points, self.rng)
        table = self._upload(torch.from_numpy(np.concatenate([sel_off, nsel, perm])))
        out = torch.empty_like(depth)
        max_sel = max(0, int(nsel.max()))
        L.check(lib.vidc_sparse_sample_scatter(L.ptr(depth), L.ptr(index), table.data_ptr() + 8 * B if perm.size else None, table.data_ptr(),
                                               table.data_ptr() + 4 * B, max_sel, B, HW, L.ptr(out), st), "sparse_sample_scatter")
        self._keep = (count, index, scratch, table)
        return out

    def __call__(self, color_u8, depth_u16, orient_u8, mask_u8, gravity, klt_tracks, predicted_normal_u8=None):
        H, W = self.out_hw
        B = len(klt_tracks)
        u8, u16 = (torch.uint8,), (torch.uint16, torch.int16)
        color = self._input(color_u8, "color_u8", u8, (B, H, W, 3))
        depth16 = self._input(depth_u16, "depth_u16", u16, (B, H, W))
        orient = self._input(orient_u8, "orient_u8", u8, (B, H, W, 3))
        mask = self._input(mask_u8, "mask_u8", u8, (B, H, W))
        gv = np.asarray(gravity, dtype=np.float64)
        if gv.shape != (B, 3):
            raise RuntimeError("gravity: shape %s, expected %s" % (gv.shape, (B, 3)))
        ga = [scannet_gravity_and_alignment(g) for g in gv]
        depth = self.gt_depth(depth16)                      # dataset.py:124-126: / 1000.0, identity tables
        if self.random_sparse:
            sparse = self.random_sparse_sample(depth, klt_tracks)
        else:
            sparse = self.pixel_tracks(klt_tracks, None if self.read_pointcloud else depth)
        out = {"image": self.decode(color, L.U8_UNIT), "mask": self.decode(mask, L.U8_UNIT).view(B, H, W), "depth": depth,
               "normal": self.decode(orient, L.U8_NORMAL_GT), "sparse_depth": sparse,
               "gravity": self._upload(torch.stack([g for g, _ in ga])), "aligned_direction": self._upload(torch.stack([a for _, a in ga])),
               "homogeneous_coordinates": self.homogeneous.unsqueeze(0).expand(B, -1, -1, -1)}
        if predicted_normal_u8 is not None:
            out["predicted_normal"] = self.decode(self._input(predicted_normal_u8, "predicted_normal_u8", u8, (B, H, W, 3)), L.U8_NORMAL_PRED)
        return out


class NYUFramePreprocessor(_TrainingBatches):
    """The batch dictionary of NYUDataset (dataset.py:381-438) on the device: image (bilinear resize + ToTensor), depth (nearest resize,
    / 5000, the [min_depth, max_depth] rule), sparse_depth and predicted_normal.

        pre = NYUFramePreprocessor(device)
        batch = pre(color_u8, depth_u16, klt_tracks, predicted_normal_u8)      # (B,480,640,3) / (B,480,640) / list of (N_i,4) / (B,240,320,3)"""

    DEPTH_UNITS_PER_METRE = 5000.0      # dataset.py:405

    def __init__(self, device="cuda", in_hw=(480, 640), out_hw=(240, 320), max_depth=7.0, min_depth=0.1):
        super().__init__(device, in_hw=in_hw, out_hw=out_hw)
        self.max_depth, self.min_depth = float(max_depth), float(min_depth)

    def gt_depth_range(self, depth_u16):
        """(B,H,W) uint16 on the device -> (B,1,Ho,Wo) float32 metres, 0 outside [min_depth, max_depth] (dataset.py:403-408)."""
        if not depth_u16.is_cuda or depth_u16.dtype not in (torch.uint16, torch.int16):
            raise RuntimeError("gt_depth_range() takes a uint16 GPU tensor (B,H,W)")
        x = depth_u16.contiguous()
        B = x.shape[0]
        H, W = self.in_hw
        Ho, Wo = self.out_hw
        y = torch.empty((B, 1, Ho, Wo), dtype=torch.float32, device=x.device)
        L.check(L.lib().vidc_resize_nearest_u16_depth_range(L.ptr(x), L.ptr(y), B, H, W, Ho, Wo, L.ptr(self.nx), L.ptr(self.ny), self.DEPTH_UNITS_PER_METRE,
                                                            self.min_depth, self.max_depth, L.current_stream()), "gt_depth_range")
        return y

    def __call__(self, color_u8, depth_u16, klt_tracks, predicted_normal_u8=None):
        (H, W), (Ho, Wo) = self.in_hw, self.out_hw
        B = len(klt_tracks)
        color = self._input(color_u8, "color_u8", (torch.uint8,), (B, H, W, 3))
        depth16 = self._input(depth_u16, "depth_u16", (torch.uint16, torch.int16), (B, H, W))
        out = {"image": self.resize(color), "depth": self.gt_depth_range(depth16), "sparse_depth": self.pixel_tracks(klt_tracks)}
        if predicted_normal_u8 is not None:
            out["predicted_normal"] = self.decode(self._input(predicted_normal_u8, "predicted_normal_u8", (torch.uint8,), (B, Ho, Wo, 3)),
                                                  L.U8_NORMAL_PRED_NYU)
        return out
