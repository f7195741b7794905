"""CPU test: the cache record of a precomputed operand (pkernels.hpp: pw_pre_pack / pw_pre_unpack,
the limb-major record k_pwsx writes and k_pwsp reads) compiled for the host
(tests/pw_pre_host/pw_pre_host_test.cpp) for M = 10, 18, 20: the meta word round-trips every
(flag, sign, P < 2 N'), and pw_mulmod on an operand that went through a record equals pw_mulmod on
the original (Lb, cb) and GMP -- 0, 1, 2^N' - 1, the flagged 2^N', 0x80 / 0x7f bytes in every
ordered pair, saturated digits and 2000 seeded random residues."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_pre_host", "pw_pre_host_test")


def test_record_roundtrip_and_mulmod_vs_gmp():
    assert os.path.exists(EXE), "tests/pw_pre_host/pw_pre_host_test not built (run __graft_entry__.build())"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    for M in (10, 18, 20):
        assert "M=%d record bad=0" % M in p.stdout, p.stdout
