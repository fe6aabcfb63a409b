"""CPU restatement of the PNG writer (include/vidc.h, `vidc_png_format` and the file layout under it): the four sample conversions in numpy
as the reference writes them (`SaveDepthsToImage` / `SaveNormalsToImage` / `SaveRgbToImage` / `SaveMasksToImage`, network_run.py:32-69) and
the file byte for byte with `struct`, `zlib.crc32` and `zlib.adler32` -- not `zlib.compress`, whose block splitting is not ours to pin."""
import struct
import zlib

import numpy as np

DEPTH16_F32, NORMAL8_F32, RGB8_F32, GRAY8_U8 = range(4)
BLOCK = 65535
# format -> (bytes per pixel, bit depth, colour type)
LAYOUT = {DEPTH16_F32: (2, 16, 0), NORMAL8_F32: (3, 8, 2), RGB8_F32: (3, 8, 2), GRAY8_U8: (1, 8, 0)}


def depth_mm(depth):
    """(H, W) float32 metres -> the uint32 millimetres of `(depths * 1000).astype(np.uint32)` (depths >= 0: the final ReLU)."""
    return (np.asarray(depth, np.float32) * np.float32(1000)).astype(np.uint32)


def depth_samples(depth):
    """... as Pillow writes a mode-I image to a 16-bit PNG: saturated to 65535."""
    return np.minimum(depth_mm(depth), 65535).astype(np.uint16)


def normal_samples(n):
    """(3, H, W) float32 -> (H, W, 3) uint8: `((1 + normals) * 127.5).astype(np.uint8)`, two rounded fp32 operations."""
    n = np.asarray(n, np.float32).transpose(1, 2, 0)
    return ((np.float32(1) + n) * np.float32(127.5)).astype(np.uint8)


def normal_samples_fused(n):
    """What a fused multiply-add (n * 127.5 + 127.5, one rounding) would give: NOT the reference's bytes everywhere."""
    n = np.asarray(n, np.float32).transpose(1, 2, 0).astype(np.float64)
    return (n * 127.5 + 127.5).astype(np.float32).astype(np.uint8)


def rgb_samples(x):
    """(3, H, W) float32 in [0, 1] -> (H, W, 3) uint8: `np.transpose(rgb * 255, [1, 2, 0]).astype(np.uint8)`."""
    return (np.asarray(x, np.float32) * np.float32(255)).transpose(1, 2, 0).astype(np.uint8)


def mask_samples(m):
    return np.asarray(m, np.uint8)


def samples(image, fmt):
    """One image in the layout of the format's source tensor -> its samples (H, W) or (H, W, 3)."""
    image = np.asarray(image)
    if fmt in (DEPTH16_F32, GRAY8_U8) and image.ndim == 3:          # (1, H, W): SaveDepthsToImage / SaveMasksToImage squeeze it
        assert image.shape[0] == 1
        image = image[0]
    return {DEPTH16_F32: depth_samples, NORMAL8_F32: normal_samples, RGB8_F32: rgb_samples, GRAY8_U8: mask_samples}[fmt](image)


def raw_scanlines(samp):
    """Samples (H, W) or (H, W, 3), uint8 or uint16 -> the bytes deflate carries: per row the filter byte 0, then the samples big-endian."""
    H = samp.shape[0]
    body = samp.astype(">u2" if samp.dtype == np.uint16 else np.uint8).reshape(H, -1).view(np.uint8)
    return np.concatenate([np.zeros((H, 1), np.uint8), body], axis=1).tobytes()


def file_bytes(H, W, fmt):
    raw = H * (1 + W * LAYOUT[fmt][0])
    return 57 + 2 + 5 * -(-raw // BLOCK) + raw + 4


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def build_png(raw, H, W, bitdepth, colourtype):
    """The file: signature, IHDR, ONE IDAT chunk of stored deflate blocks (65535 raw bytes in all but the last), IEND."""
    assert len(raw) > 0
    z = b"\x78\x01"
    for o in range(0, len(raw), BLOCK):
        blk = raw[o:o + BLOCK]
        z += struct.pack("<BHH", o + BLOCK >= len(raw), len(blk), len(blk) ^ 0xFFFF) + blk
    z += struct.pack(">I", zlib.adler32(raw))
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bitdepth, colourtype, 0, 0, 0)) + _chunk(b"IDAT", z) +
            _chunk(b"IEND", b""))


def encode(image, fmt):
    """One image (numpy, the layout of the format's source tensor) -> its file."""
    samp = samples(image, fmt)
    return build_png(raw_scanlines(samp), samp.shape[0], samp.shape[1], LAYOUT[fmt][1], LAYOUT[fmt][2])


def idat_payload(png):
    """The zlib stream of the file's IDAT chunk(s), every chunk's CRC checked on the way."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    o, z, kinds = 8, b"", []
    while o < len(png):
        n, = struct.unpack(">I", png[o:o + 4])
        kind, data = png[o + 4:o + 8], png[o + 8:o + 8 + n]
        assert struct.unpack(">I", png[o + 8 + n:o + 12 + n])[0] == zlib.crc32(kind + data), kind
        kinds.append(kind)
        if kind == b"IDAT":
            z += data
        o += 12 + n
    assert o == len(png) and kinds == [b"IHDR", b"IDAT", b"IEND"], kinds
    return z
