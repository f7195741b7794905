"""CPU test: k_pwmm's inner accumulation (pkernels.hpp: pw_mulmod products added with their signs by
pw_mm_add) compiled for the host (tests/pw_mm_host/pw_mm_host_test.cpp) for M = 10, 18, 20: sums of one to
four signed products of canonical residues -- every ordered pair of eight kinds (0, 1, 2^N' - 1, the flagged
2^N', 0x80 / 0x7f bytes, random, near 2^N') in the first two terms, both signs -- against GMP mod 2^N' + 1,
the accumulator's top inside [-2 kk, 2 kk], and pw_canon of the result."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_mm_host", "pw_mm_host_test")


def test_signed_sums_of_products_vs_gmp():
    assert os.path.exists(EXE), "tests/pw_mm_host/pw_mm_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18, 20):
        assert "M=%d sums bad=0" % M in p.stdout, p.stdout
