"""CPU test: k_pwss's inner product pw_mulmod (pkernels.hpp) compiled for the host and checked
against GMP (tests/pw_mul_host/pw_mul_host_test.cpp) for M = 10, 18, 20 -- once with the shipped
per-M switch between the schoolbook and the Karatsuba path, once with the Karatsuba path at every
M: equal halves, every order of the halves, ones against zeros, 2^N' - 1 squared, 0, 1, single
bits at N'/2 - 1, N'/2 and N' - 1, the 2^N' flags and 20 000 random pairs; the result must be
congruent mod 2^N' + 1 with its top inside the documented bound {-1, 0}."""
import os
import re
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_mul_host")


@pytest.mark.parametrize("exe", ["pw_mul_host_test", "pw_mul_host_test_kara"])
def test_mulmod_vs_gmp(exe):
    path = os.path.join(DIR, exe)
    assert os.path.exists(path), "tests/pw_mul_host/%s not built (run __graft_entry__.build())" % exe
    p = subprocess.run([path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18, 20):
        kara = 1 if exe.endswith("_kara") else "[01]"
        assert re.search(r"M=%d kara=%s mulmod bad=0 " % (M, kara), p.stdout), p.stdout
        assert "M=%d fold bad=0 " % M in p.stdout, p.stdout
