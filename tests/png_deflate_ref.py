"""CPU restatement of the compressed PNG files (include/vidc.h, the layout under `vidc_png_filter`): the five PNG filters and the adaptive
row choice in numpy, a Huffman-only dynamic deflate block with the fixed 1106-bit header in pure Python, the unrestricted Huffman optimum
with `heapq`, length-limited optimal lengths by package-merge, and a parser of such a file.  The sample conversions, the chunk framing and
`idat_payload` are those of tests/png_ref.py."""
import heapq
import struct
import zlib

import numpy as np

import png_ref as R

FILTER_NONE, FILTER_SUB, FILTER_UP, FILTER_AVERAGE, FILTER_PAETH, FILTER_ADAPTIVE = range(6)
HEADER_BITS = 1106                      # 3 + 14 + 19 * 3 + 258 * 4
MAX_BITS = 15
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def sample_bytes(samp):
    """Samples (H, W) or (H, W, 3), uint8 or uint16 -> (H, W * bpp) uint8, 16-bit samples big-endian."""
    H = samp.shape[0]
    return np.ascontiguousarray(samp.astype(">u2" if samp.dtype == np.uint16 else np.uint8)).reshape(H, -1).view(np.uint8)


def bytes_per_pixel(samp):
    return (2 if samp.dtype == np.uint16 else 1) * (3 if samp.ndim == 3 else 1)


def filter_candidates(samp):
    """(5, H, W * bpp) uint8: every row under None, Sub, Up, Average, Paeth (PNG specification 9.2-9.4; raw neighbours, zeros outside)."""
    x = sample_bytes(samp).astype(np.int32)
    bpp = bytes_per_pixel(samp)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b[1:] = x[:-1]
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def row_filters(samp, filt):
    """The filter id of every row: `filt` itself for 0..4; for FILTER_ADAPTIVE the filter with the smallest sum of |byte as int8| over the
    row's filtered bytes, ties to the lowest id."""
    H = samp.shape[0]
    if filt != FILTER_ADAPTIVE:
        assert 0 <= filt <= 4
        return np.full(H, filt, np.uint8)
    cost = np.abs(filter_candidates(samp).view(np.int8).astype(np.int64)).sum(axis=2)          # (5, H)
    return np.argmin(cost, axis=0).astype(np.uint8)                                           # the first minimum: the lowest id


def filtered_scanlines(samp, filt):
    """The bytes the deflate stream carries: per row the filter byte, then the filtered row."""
    cand, f = filter_candidates(samp), row_filters(samp, filt)
    rows = cand[f, np.arange(samp.shape[0])]
    return np.concatenate([f[:, None], rows], axis=1).tobytes()


def histogram(data):
    """257 counts: the 256 literals of `data` and one end-of-block."""
    return np.concatenate([np.bincount(np.frombuffer(data, np.uint8), minlength=256), [1]]).astype(np.int64)


def huffman_optimum(hist):
    """(cost in bits, depth) of the unrestricted Huffman code of the used symbols; among equal weights the shallowest subtree merges
    first, which gives the smallest depth an optimal code can have."""
    heap = [(int(w), 0) for w in hist if w > 0]
    assert len(heap) >= 2
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        w1, d1 = heapq.heappop(heap)
        w2, d2 = heapq.heappop(heap)
        cost += w1 + w2
        heapq.heappush(heap, (w1 + w2, max(d1, d2) + 1))
    return cost, heap[0][1]


def package_merge(hist, limit=MAX_BITS):
    """Optimal code lengths under `limit` bits (Larmore-Hirschberg), 0 for unused symbols."""
    used = [s for s in range(len(hist)) if hist[s] > 0]
    n = len(used)
    assert 2 <= n <= 1 << limit
    leaves = sorted((int(hist[s]), i) for i, s in enumerate(used))
    unit = np.eye(n, dtype=np.int64)
    items = [(w, unit[i]) for w, i in leaves]
    merged = list(items)
    for _ in range(limit - 1):
        packages = [(merged[k][0] + merged[k + 1][0], merged[k][1] + merged[k + 1][1]) for k in range(0, len(merged) - 1, 2)]
        merged = sorted(items + packages, key=lambda it: it[0])
    depth = sum(v for _, v in merged[:2 * n - 2])
    lengths = np.zeros(len(hist), np.int64)
    lengths[used] = depth
    return lengths


def flat_bits(hist):
    """ceil(log2(used symbols))."""
    return max(1, int(np.count_nonzero(hist)) - 1).bit_length()


def kraft(lengths):
    """Sum of 2^(15 - len) over the used symbols: 2^15 for a complete code."""
    return sum(1 << (MAX_BITS - int(b)) for b in lengths if b > 0)


def canonical_codes(lengths):
    """RFC 1951 3.2.2."""
    lengths = [int(b) for b in lengths]
    count = [0] * (MAX_BITS + 2)
    for b in lengths:
        count[b] += 1
    count[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for bits in range(1, MAX_BITS + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, b in enumerate(lengths):
        if b:
            codes[s] = nxt[b]
            nxt[b] += 1
    return codes


class _Bits:
    def __init__(self):
        self.bits = []

    def value(self, v, n):              # a number: least significant bit first
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):               # a Huffman code: most significant bit first
        self.bits += [(v >> i) & 1 for i in range(n - 1, -1, -1)]


def header_prefix_bits():
    """The 74 bits in front of the 258 lengths."""
    w = _Bits()
    w.value(1, 1), w.value(2, 2), w.value(0, 5), w.value(0, 5), w.value(15, 4)
    for sym in CLC_ORDER:
        w.value(4 if sym < 16 else 0, 3)
    return w.bits


def deflate_block(data, lengths):
    """`data` as ONE Huffman-only dynamic block with the fixed header, padded with zero bits to a byte."""
    assert len(lengths) == 257 and max(lengths) <= MAX_BITS and kraft(lengths) == 1 << MAX_BITS
    w = _Bits()
    w.bits = header_prefix_bits()
    for b in list(lengths) + [0]:       # ... and the one distance code, unused
        w.code(int(b), 4)
    assert len(w.bits) == HEADER_BITS
    codes = np.array(canonical_codes(lengths), np.int64)
    lens = np.asarray(lengths, np.int64)
    sym = np.concatenate([np.frombuffer(data, np.uint8).astype(np.int64), [256]])
    sl, sc = lens[sym], codes[sym]
    assert sl.min() > 0
    start = HEADER_BITS + np.concatenate([[0], np.cumsum(sl)[:-1]])
    total = HEADER_BITS + int(sl.sum())
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    bits[:HEADER_BITS] = w.bits
    for j in range(MAX_BITS):
        m = sl > j
        bits[start[m] + j] = (sc[m] >> (sl[m] - 1 - j)) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def zlib_stream(data, lengths=None):
    if lengths is None:
        lengths = package_merge(histogram(data))
    return b"\x78\x01" + deflate_block(data, lengths) + struct.pack(">I", zlib.adler32(data))


def encode(image, fmt, filt):
    """One image (numpy, the layout of the format's source tensor) -> its compressed file, with optimal lengths of at most 15 bits."""
    samp = R.samples(image, fmt)
    H, W = samp.shape[:2]
    _, bitdepth, colourtype = R.LAYOUT[fmt]
    return (b"\x89PNG\r\n\x1a\n" + R._chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bitdepth, colourtype, 0, 0, 0)) +
            R._chunk(b"IDAT", zlib_stream(filtered_scanlines(samp, filt))) + R._chunk(b"IEND", b""))


def max_file_bytes(H, W, fmt):
    raw = H * (1 + W * R.LAYOUT[fmt][0])
    return 57 + 2 + -(-(HEADER_BITS + 9 * (raw + 1)) // 8) + 4


def parse(png):
    """The fields of a compressed file: dict with `ihdr` (the 13 bytes), `payload` (the zlib stream), `prefix` (the 74 header bits in front
    of the lengths), `bfinal`, `btype`, `hlit`, `hdist`, `hclen`, `clc` (the 19 code-length-code lengths as stored), `lengths` (258),
    `data` (the inflated bytes) and `symbol_bits` (the bits of all literals and the end-of-block under `lengths`)."""
    z = R.idat_payload(png)
    assert png[12:16] == b"IHDR"
    bits = np.unpackbits(np.frombuffer(z[2:], np.uint8), bitorder="little")
    num = lambda o, n: int(sum(int(bits[o + i]) << i for i in range(n)))                       # noqa: E731
    out = {"ihdr": png[16:29], "payload": z, "prefix": [int(b) for b in bits[:74]], "bfinal": num(0, 1), "btype": num(1, 2),
           "hlit": num(3, 5), "hdist": num(8, 5), "hclen": num(13, 4), "clc": [num(17 + 3 * k, 3) for k in range(19)]}
    lengths = [int(sum(int(bits[74 + 4 * k + i]) << (3 - i) for i in range(4))) for k in range(258)]
    data = zlib.decompress(z)
    out["lengths"], out["data"] = lengths, data
    out["symbol_bits"] = int((histogram(data) * np.array(lengths[:257], np.int64)).sum())
    return out
