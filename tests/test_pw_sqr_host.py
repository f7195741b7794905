"""CPU test: the squaring kernel's inner product pw_sqrmod (pkernels.hpp, k_pwsq) compiled for
the host and checked against pw_mulmod(a, a) and GMP (tests/pw_sqr_host/pw_sqr_host_test.cpp)
for M = 10, 18, 20: 0, 1, 2^N' - 1, 2^N', 0x80 / 0x7f bytes, saturated 29-bit digits (the
column-sum bound's worst case) and 2000 seeded random residues."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_sqr_host", "pw_sqr_host_test")


def test_sqrmod_vs_mulmod_and_gmp():
    assert os.path.exists(EXE), "tests/pw_sqr_host/pw_sqr_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18, 20):
        assert "M=%d sqrmod bad=0" % M in p.stdout, p.stdout
