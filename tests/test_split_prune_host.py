"""CPU test: the split pass's per-operand zero bound and its class predicate
(mpir-fft_amd/csrc/rdispatch.hpp: rp_zero_row, rp_live_slots, rp_pair_of, rp_class_single),
compiled for the host (tests/split_prune_host/split_prune_host_test.cpp) and compared with a
brute-force model that tracks, per slot, the set of live inputs feeding it through the DIF
levels: for every group size 2..16, every level and every live count 0..G, "single" holds iff
the set has one element and the representative is the lowest partner slot with that set.  The
bound is checked against its definition (a partly filled row is live), including j an exact
multiple of NC, j = 1 and j > n."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "split_prune_host", "split_prune_host_test")


def test_split_prune_predicates_vs_model():
    assert os.path.exists(EXE), "tests/split_prune_host/split_prune_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    assert "G=8 classes bad=0" in p.stdout and "G=16 classes bad=0" in p.stdout and "bounds bad=0" in p.stdout, p.stdout
