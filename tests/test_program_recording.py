"""The engine records what it recorded when tests/golden/program_recordings.json was written: every launch descriptor of the frame
program, the stand-alone networks and DORN in the four precision modes, of the mixed frame program with VIDC_FUSE_SPLIT=0 and with
VIDC_FUSE_WARP=1, and of the first- and drain-tick group variants of the mixed frame program (tools/program_digest.py: dry-run on CPU,
device addresses replaced by stable names).  A change of the host engine
that is meant to leave the launches alone passes this unchanged; one that is meant to change them re-records the golden and says so."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import program_digest as PD  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from vi_depth_completion_amd import _lib as L
    try:
        return L.lib()
    except Exception as e:     # the library is built by __graft_entry__.build()
        pytest.skip("libvidc.so not built: %s" % e)


def test_recordings_match_the_golden(lib):
    golden = json.load(open(PD.GOLDEN))
    dumps = PD.dump_all()
    assert sorted(dumps) == sorted(golden) and len(golden) == 18
    bad = []
    for name, d in dumps.items():
        n, sha, counters, op_hashes = PD.digest(d)
        print(name, n, sha, counters)
        if [n, sha, counters, op_hashes] != golden[name]:
            first = next((i for i, (a, b) in enumerate(zip(op_hashes, golden[name][3])) if a != b), None)
            where = "op %d (%s) is the first that differs" % (first, d["ops"][first]["name"]) if first is not None else \
                "the ops in common are equal: the op count or the program's buffer sizes, cuts, allocation or counters differ"
            bad.append("%s: %d ops %s counters %s, golden %d ops %s counters %s; %s" % ((name, n, sha[:12], counters) + (
                golden[name][0], golden[name][1][:12], golden[name][2], where)))
    assert not bad, "\n".join(bad)
