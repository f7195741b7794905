"""The truncated inverse column transform's tail: the half-adds that follow a FILL step are
collapsed in the FILL store of the block IFFT's last pass (k_rpass DIR 1 mode bit 2 with
PassArgs::fill_hmin); Exec::itft_r / itft1_r skip the k_rpair<PP,1> launches the pass took.

The fix steps (d = a - b, a += d, b = 2^e d; k_rpair<PP,3>) keep their launches: as an
epilogue of the block IFFT before them they were built and measured, and the multiply got no
faster at C3 and C4 and slower at C2 (profiles/r07/fix_fold_ab.txt), so the fold was dropped.
The cases below with a fix step assert the launch and check the product around it.

Host side (no GPU): mpfft_inv_columns_schedule is a dry run of the recursion; the launch
lists of the small plans below and of the benchmark's C3 and C4 plans are checked against
what the recursion of IFFT_radix2_truncate1 (mul_fft.c:1604-1668) asks for.

GPU: whole products against GMP at the smallest plans that reach each form, l = 1024, 2048
and 4096, a random and an all-ones operand pair per shape.

Row patterns: the FILL's block has h rows (NR/2 at the top level), t' of the next h live.  Its pass's
groups hold positions `step` apart; the half-adds under the FILL have the distances h/2, h/4,
.. as long as they exceed t', and a pass takes those that are multiples of its step.
"""
import numpy as np
import pytest

# depth, w, limbs, l, FILL pass, half-adds absorbed ("d1..d0" or None), k_rpair<PP,1> launches left
# (off, h), k_rpair<PP,3> (fix) launches (off, h)
CASES = [
    # one half-add absorbed (NR 16, Tr 10: t' = 2, distance 4; the single-pass block, G = 8)
    (6, 1024, 16710, 1024, "k_rpass<3,1,1,14>", "4..4", [], []),
    (7, 1024, 66842, 2048, "k_rpass<3,2,1,14>", "4..4", [], []),
    (7, 2048, 133689, 4096, "k_rpass<3,4,1,6>", "4..4", [], []),
    # two nested half-adds absorbed (NR 32, Tr 18: t' = 2, distances 8 and 4)
    (7, 512, 33419, 1024, "k_rpass<2,1,1,4>", "8..4", [], []),       # two-pass block, step 4
    (9, 256, 262648, 2048, "k_rpass<4,2,1,14>", "8..4", [], []),     # single pass, G = 16
    (9, 512, 525316, 4096, "k_rpass<2,4,1,4>", "8..4", [], []),      # two-pass block, step 4 (C4's kernel)
    # a half-add whose distance is below the group's step: the launch stays (NR 64, Tr 34: t' = 2,
    # distances 16, 8 in the group, 4 not: step 8)
    (9, 128, 131314, 1024, "k_rpass<2,1,1,4>", "16..8", [(32, 4)], []),
    (11, 64, 1100000, 2048, "k_rpass<2,2,1,4>", "16..8", [(32, 4)], []),
    (11, 128, 2105444, 4096, "k_rpass<2,4,1,4>", "16..8", [(32, 4)], []),
    # half-adds absorbed, then a fix step (NR 64, Tr 38: t' = 6; NR 32, Tr 22)
    (9, 128, 147564, 1024, "k_rpass<2,1,1,4>", "16..8", [], [(32, 4)]),
    (9, 256, 328179, 2048, "k_rpass<4,2,1,14>", "8..8", [], [(16, 4)]),
    (9, 512, 656383, 4096, "k_rpass<2,4,1,4>", "8..8", [], [(16, 4)]),
    # a fix step followed by a half-add that no FILL precedes: both launches stay (Tr 26 of 32 or 64)
    (7, 512, 49801, 1024, "k_rpass<2,1,1,4>", None, [(24, 4)], [(16, 8)]),
    (9, 256, 197117, 2048, "k_rpass<4,2,1,14>", None, [(24, 4)], [(16, 8)]),
    (9, 512, 394249, 4096, "k_rpass<2,4,1,4>", None, [(24, 4)], [(16, 8)]),
    # no half-add follows the FILL (t' = h/2): the plain FILL store, aligned rotation round
    (7, 1024, 82570, 2048, "k_rpass<3,2,1,14>", None, [], []),
]
IDS = ["%d-%d-%d" % c[:3] for c in CASES]


def _pairs(lines, pp, op):
    out = []
    for x in lines:
        if x.startswith("k_rpair<%d,%d>" % (pp, op)):
            kv = dict(f.split("=") for f in x.split()[1:])
            out.append((int(kv["off"]), int(kv["h"])))
    return out


def _name(absorbed):
    return "k_rpass (FILL + half-add d=%s) + k_rpair" % absorbed if absorbed else "k_rpass + k_rpair"


def _check_schedule(mp, depth, w, nl, l, fpass, absorbed, hadds, fixes):
    P = mp.plan_info(nl, nl, depth, w)
    assert P["l"] == l, P
    lines = mp.inv_columns_schedule(nl, nl, depth, w)
    fill = [x for x in lines if " fill " in x]
    assert len(fill) == 1 and fill[0].startswith(fpass + " "), lines
    got = fill[0].split(" halfadd ")[1] if " halfadd " in fill[0] else None
    assert got == absorbed, lines
    assert _pairs(lines, l // 1024, 1) == hadds, lines
    assert _pairs(lines, l // 1024, 3) == fixes, lines
    assert mp.stage_kernels(nl, nl, depth, w)["inv_columns"] == _name(absorbed)
    return lines


@pytest.mark.parametrize("depth,w,nl,l,fpass,absorbed,hadds,fixes", CASES, ids=IDS)
def test_schedule_small_plans(mp, depth, w, nl, l, fpass, absorbed, hadds, fixes):
    lines = _check_schedule(mp, depth, w, nl, l, fpass, absorbed, hadds, fixes)
    # the absorbed distances are exactly those of the recursion that are multiples of the group's
    # step: redo the recursion here, from the FILL's block length h and live row count t'
    kv = dict(f.split("=") for f in [x for x in lines if " fill " in x][0].split() if "=" in f)
    h, t1 = int(kv["off"]), int(kv["lo"])
    assert 0 < t1 < h
    logg = int(fpass.split("<")[1].split(",")[0])
    step = h >> logg
    dist = []
    d = h // 2
    while d > t1:
        dist.append(d)
        d //= 2
    ins = [d for d in dist if d % step == 0]
    assert (("%d..%d" % (ins[0], ins[-1])) if ins else None) == absorbed
    assert [hh for (_, hh) in hadds if hh in dist] == [d for d in dist if d % step]


def test_schedule_c3_c4(mp):
    """The benchmark's plans.  C3 (256 rows, 156 live): both half-adds (distances 64 and 32, rows
    220..255 and 188..191) ride in the FILL store, no k_rpair<2,1> launch is left; the two fix steps
    keep their k_rpair<2,3> launches (module docstring).  C4 (512 rows, 300 live): the half-adds at
    128 and 64 ride in the FILL store; the one at off 288, h 16 follows a fix, not a FILL, and
    stays, as do the two fix steps.  C2 has no half-add under its FILL: untouched."""
    c3 = _check_schedule(mp, 15, 4, 20312500, 2048, "k_rpass<3,2,1,4>", "64..32", [], [(128, 16), (144, 8)])
    assert not [x for x in c3 if x.startswith("k_rpair<2,1>")]
    assert [x.split()[0] for x in c3] == [
        "k_rpass<4,2,1,10>", "k_rpass<3,2,1,4>", "k_rpass<4,2,1,10>", "k_rpair<2,3>", "k_rpass<3,2,1,10>",
        "k_rpair<2,3>", "k_rpass<2,2,1,10>", "k_rchain<2,1>", "k_rpair<2,5>", "k_rchain<2,2>"]
    c4 = _check_schedule(mp, 17, 2, 156250000, 4096, "k_rpass<2,4,1,4>", "128..64", [(288, 16)],
                         [(256, 32), (288, 8)])
    assert [x.split()[0] for x in c4] == [
        "k_rpass<3,4,1,2>", "k_rpass<3,4,1,0>", "k_rpass<2,4,1,4>", "k_rpass<3,4,1,2>", "k_rpass<2,4,1,0>",
        "k_rpair<4,3>", "k_rpair<4,1>", "k_rpass<3,4,1,2>", "k_rpair<4,3>", "k_rpass<2,4,1,2>",
        "k_rchain<4,1>", "k_rchain<4,1>", "k_rchain<4,2>"]
    assert mp.stage_kernels(15625000, 15625000, 15, 4)["inv_columns"] == "k_rpass + k_rpair"


@pytest.mark.gpu
@pytest.mark.parametrize("depth,w,nl,l,fpass,absorbed,hadds,fixes", CASES, ids=IDS)
def test_tail_fold_products(mp, oracle, depth, w, nl, l, fpass, absorbed, hadds, fixes):
    _check_schedule(mp, depth, w, nl, l, fpass, absorbed, hadds, fixes)
    a = mp.fill_random(nl, 0x7a11 + depth)
    b = mp.fill_random(nl, 0xf01d + w)
    assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), "random"
    ones = np.full(nl, 2**64 - 1, dtype=np.uint64)
    assert (mp.mul(ones, ones, depth, w) == oracle.gmp_mul(ones, ones)).all(), "all ones"
