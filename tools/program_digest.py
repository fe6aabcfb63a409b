"""Canonical dumps of the engine's recorded programs, for "this refactor records what its parent recorded".

    python tools/program_digest.py DIR            # the full dumps, DIR/<name>.json, for diffing two commits
    python tools/program_digest.py DIR --golden   # ... and tests/golden/program_recordings.json: {name: [ops, sha256 of the dump, counters, op hashes]}

18 dry-run recordings on CPU (batch 1, 240x320; tests/test_bf16_cpu.py::_record): the frame program, the two stand-alone networks and
-- under mixed and bf16 -- the DORN network in each of the four precision modes, the mixed frame program with VIDC_FUSE_SPLIT=0 and
with VIDC_FUSE_WARP=1, and the two group variants of the mixed frame program's segment 0 that pipeline.build_frame_program makes (the
first and the drain tick).  A dump holds every op (name, kind, stream, wait mask, buffers read and written, the whole descriptor) and the
program's buffer sizes, cuts, allocation and fold counters.  Device addresses are replaced by names that do not depend on the process:
["S", storage block, byte offset], ["K", kept weight / affine tensor, byte offset], ["WS", stream id]; an address that is none of these
is an error.  tests/test_program_recording.py compares the digests with the committed golden.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "program_recordings.json")
MODES = ("fp32", "mixed", "mxfp8", "bf16")
EXTRA = {"mixed+nofuse/frame": ("VIDC_FUSE_SPLIT", "0"), "mixed+fusewarp/frame": ("VIDC_FUSE_WARP", "1")}      # frame program, mixed mode
VARIANTS = {"mixed/frame/variant(0,1,4,keep)": (0, 0, 1, 4, True), "mixed/frame/variant(1,4,4,drop)": (0, 1, 4, 4, False)}      # Program.variant_ops arguments
COUNTERS = ("n_fused_splits", "n_fused_quants", "n_fused_casts", "n_fused_warps")
CONV_POINTERS = ("x", "w", "y", "scale1", "shift1", "scale2", "shift2", "residual", "workspace", "y_split")


def record_all(programs=None):
    """{"<mode>/<name>": Program} of the 16 whole-program recordings.  programs: {mode: _record(mode)} the caller made already."""
    from test_bf16_cpu import _record
    out = {}
    for mode in MODES:
        for name, prog in (programs[mode] if programs is not None else _record(mode)).items():
            out["%s/%s" % (mode, name)] = prog
    for name, (var, value) in EXTRA.items():
        old = os.environ.get(var)
        os.environ[var] = value
        try:
            out[name] = _record("mixed")["frame"]
        finally:
            if old is None:
                os.environ.pop(var)
            else:
                os.environ[var] = old
    return out


def _namer(prog):
    """address -> its stable name."""
    blocks, kept = [], []           # (first byte, end, index)
    for seen, tensors, table in ((set(), prog.storage, blocks), (set(), prog._keep, kept)):
        for t in tensors:
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                table.append((t.data_ptr(), t.data_ptr() + max(t.numel() * t.element_size(), 1), len(table)))
    spaces = {t.data_ptr(): sid for sid, t in prog.workspaces.items()}

    def name(a):
        if not a:
            return None
        if a in spaces:
            return ["WS", spaces[a]]
        for tag, table in (("S", blocks), ("K", kept)):
            for lo, hi, k in table:
                if lo <= a < hi:
                    return [tag, k, a - lo]
        raise ValueError("address 0x%x is in no storage block, kept tensor or workspace of the program" % a)
    return name


def dump_all():
    """{name: dump} of the 18 recordings."""
    progs = record_all()
    dumps = {name: dump(prog) for name, prog in progs.items()}
    for name, args in VARIANTS.items():
        dumps[name] = dump(progs["mixed/frame"], *progs["mixed/frame"].variant_ops(*args))
    return dumps


def dump(prog, c_ops=None, indices=None):
    """The canonical form of a finalized (dry-run) program: a JSON-able dict.  c_ops, indices: the op array of a group variant and the
    program's ops it was made from (Program.variant_ops), in place of the program's own."""
    from vi_depth_completion_amd import _lib as L
    name = _namer(prog)
    ops = []
    c_ops = prog.c_ops if c_ops is None else c_ops
    indices = range(len(prog.ops)) if indices is None else indices
    for cop, i in zip(c_ops, indices):
        _kind, reads, writes, _kw = prog.ops[i]
        o = {"name": prog.op_names[i], "kind": cop.kind, "stream_id": cop.stream_id, "wait_mask": cop.wait_mask,
             "reads": sorted(reads), "writes": sorted(writes)}
        if cop.kind == L.OP_CONV:
            o["conv"] = {f: (name(getattr(cop.u.conv, f)) if f in CONV_POINTERS else getattr(cop.u.conv, f)) for f, _t in L.ConvDesc._fields_}
        else:
            o["p"], o["i"], o["f"] = [name(a) for a in cop.u.g.p], list(cop.u.g.i), [repr(v) for v in cop.u.g.f]
        ops.append(o)
    assert len(ops) == len(c_ops) == len(indices) and len(prog.c_ops) == len(prog.ops) == len(prog.op_names)
    return {"ops": ops, "buf_elems": list(prog.buf_elems), "cuts": list(prog.cuts), "bytes_allocated": prog.bytes_allocated,
            "counters": {c: getattr(prog, c, 0) for c in COUNTERS}}


def text(d):
    return json.dumps(d, sort_keys=True, indent=1)


def digest(d):
    """[op count, sha256 of the dump, the four counters, a short hash per op] -- one entry of the golden file (the per-op hashes let the
    test name the first op that differs)."""
    return [len(d["ops"]), hashlib.sha256(text(d).encode()).hexdigest(), [d["counters"][c] for c in COUNTERS],
            [hashlib.sha256(text(o).encode()).hexdigest()[:12] for o in d["ops"]]]


def main(argv):
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    os.makedirs(argv[0], exist_ok=True)
    golden = {}
    for name, d in dump_all().items():
        golden[name] = digest(d)
        with open(os.path.join(argv[0], name.replace("/", "_") + ".json"), "w") as f:
            f.write(text(d) + "\n")
        print(name, *golden[name][:3])
    if "--golden" in argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write(text(golden) + "\n")
        print("wrote", GOLDEN)


if __name__ == "__main__":
    main(sys.argv[1:])
