"""CPU test: the carry chains around k_pwss's inner product (pkernels.hpp: pw_canon, pw_sqrt2)
compiled for the host and checked against GMP (tests/pw_chain_host/pw_chain_host_test.cpp) for
M = 10, 18, 20.  pw_canon must give the residue of L - T mod 2^N' + 1 in [0, 2^N'] with its flag
exactly for 2^N', in its common form (the low word takes T) and in its branch-free form alike;
pw_sqrt2 must give (2^(N'/2) - 1)(L + T 2^N') with the new top inside |T| + 3.  Inputs: 0, 1,
2^N' - 1, a low word of 0 and 0xffffffff under T = -3 .. 3, all-ones halves, nearly equal halves
and 20 000 random values; the common path, the wrapped low word, the 2^N' flag and pw_sqrt2's
rippled carry must each have been reached."""
import os
import re
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_chain_host", "pw_chain_host_test")


def test_chains_vs_gmp():
    assert os.path.exists(EXE), "tests/pw_chain_host/pw_chain_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18, 20):
        m = re.search(r"M=%d bad=0 canon: common path (\d+), wrapped low word (\d+), 2\^N' (\d+); "
                      r"sqrt2: rippled carry (\d+), \|T'\| - \|T\| <= (-?\d+)" % M, p.stdout)
        assert m, p.stdout
        common, wrapped, flags, ripple, td = map(int, m.groups())
        assert common > 0 and wrapped > 0 and flags > 0 and ripple > 0 and td <= 3, p.stdout
