"""CPU test: the grouped forms of k_pwss's rotated add (pw_combine GRP, pkernels.hpp: one wrap test,
base select and mask select per two consecutive partner words, the word past the wrap read from
row 2M = ~row 0; and per four, rows 2M .. 2M+2 = ~rows 0 .. 2) compiled for the host and compared bit for bit -- limbs, top and sign flag --
with the per-word pw_combine<M, LK> on the same exchange buffer
(tests/pw_pair_host/pw_pair_host_test.cpp), at M = 10 and 18, LK = 8:
every rotation E in [0, 2N') at M = 10 and, at M = 18, every E whose word offset Yw is -1, 0, 1,
2M-2 or 2M-1, every E == 0 or 31 mod 32 and 10^4 random E; each with both sign flags, alpha in
{-1, 0, 1}, partner tops {-1, 0, -2, 1} and partner words all zero, all ones, word 0 = 0 with word
1 = ~0, the reverse, and random; with the full and the kernels' bounded prefetch window.  A wrong
row 2M must change the result at every rotation whose wrap falls inside a pair.  The groups of four
(the shipped form): every rotation at both M with every pattern, and wrong rows 2M, 2M+2 noticed."""
import os
import re
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_pair_host", "pw_pair_host_test")


def test_paired_combine_equals_per_word():
    assert os.path.exists(EXE), "tests/pw_pair_host/pw_pair_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18):
        for form in ("pair", "quad"):   # quad: the groups of four (the shipped K = 256 form, pw_group)
            assert re.search(r"M=%d %s combine cases=\d+ bad=0 wrong_row_unnoticed=0" % (M, form), p.stdout), p.stdout
