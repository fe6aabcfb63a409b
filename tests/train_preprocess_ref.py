"""Host restatement of the per-frame arithmetic of the reference's two training loaders -- ScanNetSmallFramesDataset.__getitem__
(dataset.py:95-247) and NYUDataset.__getitem__ (dataset.py:381-438) -- on in-memory arrays instead of files: numpy, torch CPU and
Pillow only.  TEST INFRASTRUCTURE (tests/test_train_preprocess.py, tools/train_loader_bench.py's host leg); the product path
(vi_depth_completion_amd/preprocess.py + csrc/train_preprocess.hip) never imports it.

`skimage.io.imread` of a PNG is the decoded array, `transforms.ToTensor` is restated as in tests/test_preprocess.py, `np.float` (gone
from numpy) is float64.  Restricted to the keys main.py:262-280 and network_run.py:150-225 read."""
import numpy as np
import torch

SCANNET_FC = np.array([577.87061, 580.25851]) / 2      # dataset.py:91
SCANNET_CC = np.array([319.87654, 239.87603]) / 2      # dataset.py:92


def to_tensor(pic):
    """transforms.ToTensor on an ndarray: (H,W,C) or (H,W) -> (C,H,W); uint8 is converted to float and divided by 255, a float array
    keeps its values."""
    a = np.asarray(pic)
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    return t.float().div(255) if t.dtype == torch.uint8 else t


# ---- the literal sequences, one per tensor -------------------------------------------------------------------------------------------
def color_literal(color_img):
    """dataset.py:122-123."""
    return to_tensor(color_img)


def mask_literal(mask_img):
    """dataset.py:128-129: a float64 division, then torch.Tensor's round to float32."""
    return torch.Tensor(np.asarray(mask_img) / 255.0)


def normal_gt_literal(orient_img):
    """dataset.py:130-131."""
    return -to_tensor(orient_img) + 0.5


def predicted_normal_scannet_literal(normal_img):
    """dataset.py:219-221."""
    normal_values = 1 - np.asarray(normal_img).astype(np.float32) / 127.5
    return to_tensor(normal_values)


def predicted_normal_nyu_literal(normal_img):
    """dataset.py:394-395."""
    normal_values = 1 - np.asarray(normal_img).astype(np.float32) / 127.5
    return -to_tensor(normal_values) + 0.5


def scannet_depth_literal(depth_img):
    """dataset.py:124-126: float64 division, .float(), view(1,H,W)."""
    depth_tensor = torch.tensor(np.asarray(depth_img) / 1000.0).float()
    return depth_tensor.view(1, depth_tensor.shape[0], depth_tensor.shape[1])


# ---- the fp32 restatement the kernels follow -------------------------------------------------------------------------------------------
def decode_u8(u8, mode):
    """The four byte expressions of vidc_u8_decode_chw in torch CPU fp32, one rounding per operation: (H,W,C) or (H,W) uint8 -> (C,H,W)."""
    a = np.asarray(u8)
    if a.ndim == 2:
        a = a[:, :, None]
    x = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float()
    if mode == 0:
        return x / 255
    if mode == 1:
        return -(x / 255) + 0.5
    if mode == 2:
        return 1 - x / 127.5
    if mode == 3:
        return -(1 - x / 127.5) + 0.5
    raise ValueError(mode)


def depth_fp32(depth_u16, divisor):
    """uint16 -> float32, divided in fp32 (what vidc_resize_nearest_u16_depth computes per pixel)."""
    return torch.from_numpy(np.asarray(depth_u16).astype(np.float32)) / divisor


def compute_alignment_tensor(gravity_tensor):
    """dataset.py:45-55."""
    psi = gravity_tensor[1] * gravity_tensor[1] + gravity_tensor[2] * gravity_tensor[2]
    if psi < 1e-6:
        alignment_tensor = gravity_tensor
    else:
        pitch_angle = torch.atan2(gravity_tensor[2], gravity_tensor[1])
        if torch.cos(pitch_angle) > 0.3:
            alignment_tensor = torch.tensor([0., 1., 0.], dtype=torch.float)
        else:
            alignment_tensor = gravity_tensor
    return alignment_tensor


def pixel_tracks(klt_tracks, H, W, gt=None):
    """dataset.py:204-212 (ScanNet) and dataset.py:410-419 (NYU): the same rule -- coordinates / 2 in float64, truncated toward zero,
    later tracks overwrite earlier ones; the value is the track's depth, or with `gt` (H,W) the ground truth at that pixel.  A
    quotient that is not finite or beyond int32 is no pixel (astype(np.int32) of such a value is undefined; int() raises or is huge).
    rows (id, x, y, d) -> float32 (1,H,W)."""
    out = torch.zeros(1, H, W)
    tr = np.atleast_2d(np.asarray(klt_tracks, dtype=np.float64))
    if tr.size == 0:
        return out
    for i in range(tr.shape[0]):
        qx, qy = tr[i, 1] / 2, tr[i, 2] / 2
        if not (np.isfinite(qx) and np.isfinite(qy) and abs(qx) < 2 ** 31 and abs(qy) < 2 ** 31):
            continue
        row, col = int(qy), int(qx)
        if 0 <= row < H and 0 <= col < W:
            out[0, row, col] = float(gt[row, col]) if gt is not None else tr[i, 3]
    return out


def random_sparse(depth_tensor, num_points, rng):
    """dataset.py:191-202 with `rng` in np.random's place.  depth_tensor (1,H,W) -> (1,H,W)."""
    klt_depth_tensor = torch.zeros_like(depth_tensor)
    rows, cols = torch.nonzero(depth_tensor.squeeze(), as_tuple=True)
    if num_points >= rows.nelement():
        klt_depth_tensor = depth_tensor.clone()
    else:
        indices = rng.permutation(rows.shape[0])[0:num_points]
        klt_depth_tensor[0, rows[indices], cols[indices]] = depth_tensor[0, rows[indices], cols[indices]]
    return klt_depth_tensor


def homogeneous_coordinates(fc, cc, W, H):
    """dataset.py:34-42."""
    hom = np.zeros((H, W, 3))
    hom[:, :, 2] = 1
    xx, yy = np.meshgrid([i for i in range(0, W)], [i for i in range(0, H)])
    hom[:, :, 0] = (xx - cc[0]) / fc[0]
    hom[:, :, 1] = (yy - cc[1]) / fc[1]
    return torch.from_numpy(hom.astype(np.float32))


def scannet_item(color_img, depth_img, orient_img, mask_img, gravity, klt_tracks, predicted_normal_img=None, read_pointcloud=True,
                 random_sparse_pointcloud=False, rng=np.random, homogeneous=None):
    """ScanNetSmallFramesDataset.__getitem__ (dataset.py:95-247) from the decoded file contents; klt_tracks as np.atleast_2d(np.loadtxt(.))
    or the np.zeros((0, 4)) of a failed read."""
    H, W = np.asarray(depth_img).shape
    depth_tensor = scannet_depth_literal(depth_img)
    gravity_tensor = torch.tensor(np.asarray(gravity, dtype=np.float64), dtype=torch.float)      # dataset.py:132
    klt_tracks = np.atleast_2d(np.asarray(klt_tracks, dtype=np.float64))
    if random_sparse_pointcloud:
        sparse = random_sparse(depth_tensor, klt_tracks.shape[0], rng)
    else:
        sparse = pixel_tracks(klt_tracks, H, W, None if read_pointcloud else depth_tensor[0])
    out = {"image": color_literal(color_img), "mask": mask_literal(mask_img), "depth": depth_tensor, "gravity": gravity_tensor,
           "normal": normal_gt_literal(orient_img), "sparse_depth": sparse, "aligned_direction": compute_alignment_tensor(gravity_tensor),
           "homogeneous_coordinates": homogeneous if homogeneous is not None else homogeneous_coordinates(SCANNET_FC, SCANNET_CC, W, H)}
    if predicted_normal_img is not None:
        out["predicted_normal"] = predicted_normal_scannet_literal(predicted_normal_img)
    return out


def nyu_depth_literal(depth_img, out_wh=(320, 240), min_depth=0.1, max_depth=7.0):
    """dataset.py:403-408 on an in-memory 16-bit image."""
    from PIL import Image
    img = Image.fromarray(np.ascontiguousarray(depth_img).astype(np.uint16)).convert("F")
    img = img.resize(out_wh, resample=Image.NEAREST)
    depth_tensor = torch.Tensor(np.array(img)) / 5000.0
    depth_tensor = depth_tensor.view(1, depth_tensor.shape[0], depth_tensor.shape[1])
    depth_tensor[depth_tensor < min_depth] = 0
    depth_tensor[depth_tensor > max_depth] = 0
    return depth_tensor


def nyu_item(color_img, depth_img, klt_tracks, predicted_normal_img=None, out_wh=(320, 240), min_depth=0.1, max_depth=7.0):
    """NYUDataset.__getitem__ (dataset.py:381-438) from the decoded file contents; klt_tracks: the rows of the point file."""
    from PIL import Image
    color = Image.fromarray(np.ascontiguousarray(color_img)).resize(out_wh, resample=Image.BILINEAR)      # dataset.py:398-400
    out = {"image": to_tensor(np.asarray(color)), "depth": nyu_depth_literal(depth_img, out_wh, min_depth, max_depth),
           "sparse_depth": pixel_tracks(klt_tracks, out_wh[1], out_wh[0])}
    if predicted_normal_img is not None:
        out["predicted_normal"] = predicted_normal_nyu_literal(predicted_normal_img)
    return out


def collate(items):
    """torch's default collate of the tensors: one stack per key."""
    return {k: torch.stack([it[k] for it in items]) for k in items[0]}
