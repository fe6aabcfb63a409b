"""The evaluation outputs as PNG files (`--save`, network_run.py:32-69, 261-292), encoded on the device.

`PngEncoder` turns batches of depth maps, normal maps, RGB images and masks into complete PNG files in device memory (csrc/png.hip: stored
deflate blocks, Adler-32 and CRC-32 folded from per-segment partial sums, two launches per batch; csrc/png_deflate.hip: a PNG filter per row
and one Huffman-coded deflate block, four launches per batch, files 2 to 5 times smaller); `EvaluationWriter` is the harness's
`--save` side on top of it: the files of a batch go to a ring of pinned host buffers with one non-blocking copy each, and one thread
waits for the copy and writes them, so the thread that drives the device never waits for a file.  The layout and the conversions are
stated in include/vidc.h (`vidc_png_format`); inputs outside the stated ranges are clamped, NaN becomes 0."""
import os
import queue
import threading

import torch

from . import _lib as L


class PngEncoder:
    """Batches of images -> (B, file_stride) uint8 device tensors holding one PNG file per row, on the current stream.  The scratch of
    a (B, H, W, format) is allocated once and shared by the calls in stream order: use one encoder per stream."""

    def __init__(self, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("PngEncoder needs a GPU: the HIP path has no CPU fallback")
        self.device = torch.device(device)
        self._scratch = {}

    @staticmethod
    def file_bytes(H, W, fmt):
        n = L.lib().vidc_png_file_bytes(H, W, fmt)
        if n == 0:
            raise RuntimeError("no PNG file for a %dx%d image of format %d" % (H, W, fmt))
        return n

    @staticmethod
    def max_file_bytes(H, W, fmt):
        n = L.lib().vidc_png_deflate_max_file_bytes(H, W, fmt)
        if n == 0:
            raise RuntimeError("no PNG file for a %dx%d image of format %d" % (H, W, fmt))
        return n

    @staticmethod
    def _source(src, fmt):
        """The checks of a source tensor -> (contiguous tensor, B, H, W)."""
        want = torch.uint8 if fmt == L.PNG_GRAY8_U8 else torch.float32
        if not (torch.is_tensor(src) and src.is_cuda):
            raise RuntimeError("PngEncoder takes GPU tensors: the HIP path has no CPU fallback")
        if src.dtype != want:
            raise RuntimeError("PNG format %d takes a %s tensor, got %s" % (fmt, want, src.dtype))
        planes = 3 if fmt in (L.PNG_NORMAL8_F32, L.PNG_RGB8_F32) else 1
        if src.dim() == 4 and src.shape[1] == planes:
            B, _, H, W = src.shape
        elif src.dim() == 3 and planes == 1:
            B, H, W = src.shape
        else:
            raise RuntimeError("PNG format %d takes a (B,%d,H,W) tensor, got %s" % (fmt, planes, tuple(src.shape)))
        return src.contiguous(), B, H, W

    def _buffers(self, key, scratch_bytes, B, n, out, device):
        """The (B, stride) file buffer (`out`, checked, or a new one of n bytes per row rounded up to 16) and the scratch kept under `key`."""
        if out is None:
            out = torch.empty((B, (n + 15) // 16 * 16), dtype=torch.uint8, device=device)
        elif not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == B and out.is_contiguous()):
            raise RuntimeError("out must be a contiguous (B, stride) uint8 GPU tensor")
        scratch = self._scratch.get(key)
        if scratch is None:
            scratch = self._scratch[key] = torch.empty(scratch_bytes(), dtype=torch.uint8, device=device)
        return out, scratch

    def encode(self, src, fmt, out=None):
        """src: the format's source tensor on the device -- (B,1,H,W) / (B,H,W) float32 (depth), (B,3,H,W) float32 (normals, RGB) or (B,H,W) /
        (B,1,H,W) uint8 (mask).  Returns (files, file_bytes): row i of `files` starts with the file of image i.  out: a contiguous (B, stride)
        uint8 device tensor to encode into, stride a multiple of 16 and at least file_bytes; what lies behind a file is left as it is."""
        src, B, H, W = self._source(src, fmt)
        n = self.file_bytes(H, W, fmt)
        out, scratch = self._buffers((B, H, W, fmt), lambda: L.lib().vidc_png_scratch_bytes(B, H, W, fmt), B, n, out, src.device)
        L.check(L.lib().vidc_png_encode(L.ptr(src), B, H, W, fmt, L.ptr(out), out.shape[1], L.ptr(scratch), L.current_stream()), "png_encode")
        return out, n

    def encode_compressed(self, src, fmt, filter=L.PNG_FILTER_ADAPTIVE, out=None):
        """The same images as compressed files (a PNG filter per row: L.PNG_FILTER_NONE .. PAETH for every row, ADAPTIVE chosen per row; one
        Huffman-coded deflate block).  Returns (files, sizes): row i of `files` starts with the file of image i, sizes a (B,) uint32 device
        tensor of the files' bytes -- they depend on the images, so only the device knows them.  out: as for encode(), its stride at least
        max_file_bytes; what lies behind max_file_bytes rounded up to 16 is left as it is."""
        src, B, H, W = self._source(src, fmt)
        n = self.max_file_bytes(H, W, fmt)
        out, scratch = self._buffers((B, H, W, fmt, "deflate"), lambda: L.lib().vidc_png_deflate_scratch_bytes(B, H, W, fmt), B, n, out, src.device)
        sizes = torch.empty(B, dtype=torch.uint32, device=src.device)
        L.check(L.lib().vidc_png_encode_deflate(L.ptr(src), B, H, W, fmt, int(filter), L.ptr(out), out.shape[1], L.ptr(sizes), L.ptr(scratch),
                                                L.current_stream()), "png_encode_deflate")
        return out, sizes

    def encode_depth(self, depth):
        """Metres -> 16-bit gray: `(depths * 1000).astype(np.uint32)` as Pillow writes it (saturated to 65535)."""
        return self.encode(depth, L.PNG_DEPTH16_F32)

    def encode_normals(self, n):
        """`((1 + normals) * 127.5).astype(np.uint8)` -> 8-bit RGB."""
        return self.encode(n, L.PNG_NORMAL8_F32)

    def encode_rgb(self, x):
        """`(rgb * 255).astype(np.uint8)` -> 8-bit RGB."""
        return self.encode(x, L.PNG_RGB8_F32)

    def encode_mask(self, m):
        return self.encode(m, L.PNG_GRAY8_U8)


class _Slot:
    def __init__(self):
        self.host = None                    # pinned uint8 buffer, grown on demand
        self.free = threading.Event()
        self.free.set()


class EvaluationWriter:
    """`--save`: <save_dir>/evaluation_output/{depth,normal}_{pred,gt}_%06d.png (network_run.py:261-308).

    Every call encodes its batch on the current stream into one of `slots` pinned host buffers (non-blocking copies), records an event and
    hands both to the writer thread, which waits for the event and writes the files.  The calling thread waits only when all slots are
    still being written.  flush() returns when every file handed over so far is on disk and re-raises what the thread ran into.

    compress=True writes the compressed files of PngEncoder.encode_compressed: their sizes travel to the slot with the files, and the
    thread reads them once the event has passed."""

    def __init__(self, save_dir, slots=4, device="cuda", compress=False):
        self.encoder = PngEncoder(device)
        self.compress = bool(compress)
        self.output_path = os.path.join(save_dir, "evaluation_output")
        os.makedirs(self.output_path, exist_ok=True)
        self._slots = [_Slot() for _ in range(max(1, int(slots)))]
        self._next = 0
        self._jobs = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name="vidc-png-writer", daemon=True)
        self._thread.start()

    # ---- the two entry points of the harness ---------------------------------------------------------------------------------------
    def save_pred_only(self, sample_batched, pred_depths):
        """`_network_save_cnn_output_pred_only` (:284-292): depth_pred_%06d.png, numbered by the frame's own colour file name."""
        idx = [int(name[6:12]) for name in sample_batched["color_filename"][:pred_depths.shape[0]]]
        self._submit([("depth_pred_", pred_depths, L.PNG_DEPTH16_F32)], idx)

    def save_evaluation_output(self, sample_batched, pred_depths, start_index, pred_normals=None):
        """`_network_save_cnn_evaluation_output` (:261-282): predictions and ground truth, numbered start_index + i.  The normals (the
        prediction too, as the reference's F.normalize) pass through torch.ops.vidc.normalize_nchw first."""
        from . import torch_ops  # noqa: F401  (registers torch.ops.vidc)
        dev = self.encoder.device
        groups = []
        if pred_normals is not None:
            groups += [("normal_pred_", torch.ops.vidc.normalize_nchw(pred_normals), L.PNG_NORMAL8_F32),
                       ("normal_gt_", torch.ops.vidc.normalize_nchw(sample_batched["normal"].to(dev, non_blocking=True)), L.PNG_NORMAL8_F32)]
        groups += [("depth_pred_", pred_depths, L.PNG_DEPTH16_F32),
                   ("depth_gt_", sample_batched["depth"].to(dev, non_blocking=True)[:pred_depths.shape[0]], L.PNG_DEPTH16_F32)]
        self._submit(groups, [start_index + i for i in range(pred_depths.shape[0])])

    # ---- ring ----------------------------------------------------------------------------------------------------------------------
    def _submit(self, groups, indices):
        self._raise()
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        slot.free.wait()                    # only when the ring is full: its files of `slots` calls ago are still being written
        self._raise()
        encode = self.encoder.encode_compressed if self.compress else self.encoder.encode
        encoded = [(prefix,) + encode(t, fmt) for prefix, t, fmt in groups]
        need = sum(files.numel() + (4 * files.shape[0] if self.compress else 0) for _, files, _ in encoded)
        if slot.host is None or slot.host.numel() < need:
            slot.host = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        files_out, off = [], 0
        for prefix, files, n in encoded:
            view = slot.host[off:off + files.numel()].view(files.shape)
            view.copy_(files, non_blocking=True)
            off += files.numel()                # rows of a multiple of 16 bytes: `off` stays a multiple of 4 for the sizes behind them
            if self.compress:                   # n: the sizes on the device; the thread reads the slot's copy after the event
                sizes = slot.host[off:off + 4 * files.shape[0]].view(torch.uint32)
                sizes.copy_(n, non_blocking=True)
                off += 4 * files.shape[0]
            for i, index in enumerate(indices[:files.shape[0]]):
                files_out.append((os.path.join(self.output_path, "%s%06d.png" % (prefix, index)), view[i], sizes[i] if self.compress else n))
        event = torch.cuda.Event()
        event.record()
        slot.free.clear()
        self._jobs.put((slot, event, files_out))

    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            slot, event, files_out = job
            try:
                event.synchronize()
                for path, view, n in files_out:
                    with open(path, "wb") as f:
                        f.write(memoryview(view.numpy())[:int(n)])
            except BaseException as e:      # handed to the calling thread by _raise()
                if self._error is None:
                    self._error = e
            finally:
                slot.free.set()
                self._jobs.task_done()

    def _raise(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise RuntimeError("writing the evaluation output failed") from e

    def flush(self):
        self._jobs.join()
        self._raise()

    def close(self):
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = None
            self._raise()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
