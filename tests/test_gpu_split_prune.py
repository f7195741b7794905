"""GPU tests of the pruned split pass: k_rpass MODE 2 (FFT_split_bits fused into the first
forward column pass) with each operand's own zero bound (PassArgs::zero_op = the first row the
operand does not reach, rp_zero_row), zero-partner copies at every level and one publish per
single class (rp_class_single).

Shapes: the (depth, w) at which the fused split runs in k_rpass, from l = 1024 with NR = 8 up
to the l = 2048 / 4096 shapes of tests/test_gpu_parity.py's BIG_SHAPES; every k_rpass<LOGG,PP,0,2>
instance the library builds is reached (asserted below).  Operand sizes per shape, each class
verified on the CPU from the plan mp.plan_info returns:
  short     both operands fill about 5/16 of the rows (the flagship's pattern)
  skew      operand 1 fills more than half the rows, operand 2 one row
  one_limb  n2 = 1 limb, n1 the largest that fits with it
  boundary  operand 1 ends exactly on a row boundary (j1 a multiple of NC)
  past      operand 1 ends one coefficient past a row boundary
  largest   the largest balanced operands the shape admits
  tiny      j1 = NC + 1, j2 = 3: one or two live slots per group, the smallest truncation
Operand contents: all-ones, and random with the last live row all-ones (a wrongly pruned row
changes the product and the forward stage).

Checks: mp.mul == GMP for both contents at every case; run_stages (tests/gpu_stages.py: the
forward stage, the inverse and the combine against exact integer math) where its pure-Python
oracle stays within a few seconds.  That oracle reduces one 2N-bit value mod 2^N + 1 per slot
and operand with Python's quadratic division, 13 ms at l = 2048 and 50 ms at l = 4096, so its
cost is T N^2 whatever the operands hold: cases over STAGE_COST_MAX (T > 160 at l = 2048, T > 40
at l = 4096) take the product check only, and the "tiny" class keeps a stage check at every
shape.  The pointwise stage's own check (one more such division per slot) is left to
tests/test_gpu_parity.py: nothing here changes that stage, and the inverse and combine checks
behind it fail if it were wrong."""
import re

import numpy as np
import pytest

from helpers import max_limbs, to_int, valid_shape

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4096), (5, 2048), (5, 4096), (6, 4096), (7, 1024), (7, 2048), (8, 512), (9, 256)]
CLASSES = ["short", "skew", "one_limb", "boundary", "past", "largest", "tiny"]
STAGE_COST_MAX = 2.8e12   # T N^2: about 4 s of the stage oracle's divisions
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _limbs_upto(j, bits1):
    """the most limbs an operand of exactly j coefficients can have"""
    return (j * bits1) // 64


def _limbs_from(j, bits1):
    """the fewest limbs an operand of exactly j coefficients can have"""
    return ((j - 1) * bits1) // 64 + 1


def _zrow(j, NC):
    return -(-j // NC)


def _split_instance(mp, n1, n2, depth, w):
    """(LOGG, PP) of the k_rpass<LOGG,PP,0,2> that splits; fails when another kernel does"""
    name = mp.stage_kernels(n1, n2, depth, w)["fwd_columns"]
    m = re.search(r"k_rpass<(\d+),(\d+),0,2>", name)
    assert m, f"fused split not in k_rpass at depth {depth} w {w} n1 {n1} n2 {n2}: {name!r}"
    return int(m.group(1)), int(m.group(2))


def _case(mp, depth, w, cls):
    """(n1, n2) of the class at this shape, checked against the plan the library makes for it"""
    n = 1 << depth
    bits1 = (n * w - depth) // 2
    mx = max_limbs(depth, w)

    def plan(n1, n2):
        assert valid_shape(depth, w, n1, n2), (depth, w, n1, n2)
        P = mp.plan_info(n1, n2, depth, w)
        assert P["bits1"] == bits1 and P["NC"] * P["NR"] == 2 * n, P
        return P

    def settle(f):
        """f(NC) -> (n1, n2); the plan's column count may depend on the sizes: iterate to a fixed point"""
        NC = plan(mx // 2, mx // 2)["NC"]
        for _ in range(4):
            n1, n2 = f(NC)
            P = plan(n1, n2)
            if P["NC"] == NC:
                return n1, n2, P
            NC = P["NC"]
        raise AssertionError(f"no stable plan for {cls} at depth {depth} w {w}")

    if cls == "short":      # j = 5n/8 coefficients each: rows [0, 5 NR / 16)
        n1, n2, P = settle(lambda NC: (_limbs_upto(5 * n // 8, bits1), _limbs_from(5 * n // 8, bits1)))
        for j in (P["j1"], P["j2"]):
            assert 4 * P["NR"] <= 16 * _zrow(j, P["NC"]) <= 6 * P["NR"], P
    elif cls == "skew":     # operand 1 past half the rows, operand 2 inside row 0
        n1, n2, P = settle(lambda NC: (_limbs_upto(n + n // 2, bits1), _limbs_upto(max(1, NC // 2), bits1)))
        assert 2 * _zrow(P["j1"], P["NC"]) > P["NR"] and _zrow(P["j2"], P["NC"]) == 1 and P["j1"] > n, P
    elif cls == "one_limb":
        n1, n2, P = settle(lambda NC: (_limbs_upto(2 * n - 1, bits1), 1))
        assert P["j2"] == 1 and P["j1"] == 2 * n - 1, P
    elif cls == "boundary":  # j1 = r NC exactly, r = NR / 4 + 1; operand 2 a row and a half
        n1, n2, P = settle(lambda NC: (_limbs_upto((2 * n // NC // 4 + 1) * NC, bits1), _limbs_upto(NC + NC // 2, bits1)))
        assert P["j1"] % P["NC"] == 0 and _zrow(P["j1"], P["NC"]) == P["NR"] // 4 + 1, P
    elif cls == "past":      # j1 = r NC + 1: row r holds one coefficient
        n1, n2, P = settle(lambda NC: (_limbs_from((2 * n // NC // 4 + 1) * NC + 1, bits1), _limbs_upto(NC + NC // 2, bits1)))
        assert P["j1"] % P["NC"] == 1 and _zrow(P["j1"], P["NC"]) == P["NR"] // 4 + 2, P
    elif cls == "tiny":
        n1, n2, P = settle(lambda NC: (_limbs_from(NC + 1, bits1), _limbs_upto(3, bits1)))
        assert P["j1"] == P["NC"] + 1 and P["j2"] == 3 and P["trunc"] == 2 * P["NC"], P
    else:
        n1 = n2 = mx
        P = plan(n1, n2)
        assert not valid_shape(depth, w, mx + 1, mx + 1)
    return n1, n2, P


def _last_row_ones(mp, nl, j, NC, bits1, seed):
    """random limbs, the operand's last live row (coefficients (z - 1) NC ...) all-ones to its end"""
    a = mp.fill_random(nl, seed)
    z = _zrow(j, NC)
    a[((z - 1) * NC * bits1) // 64:] = ONES
    return a


def test_every_split_instance_is_reached(mp):
    """the shapes and classes below reach every k_rpass<LOGG,PP,0,2> instance (host-side query)"""
    seen = set()
    for depth, w in SHAPES:
        for cls in CLASSES:
            n1, n2, _ = _case(mp, depth, w, cls)
            seen.add(_split_instance(mp, n1, n2, depth, w))
    assert {(4, 2), (3, 4), (3, 2), (2, 4), (2, 2), (2, 1), (3, 1)} <= seen, seen


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("depth,w", SHAPES)
def test_split_prune_exact(mp, oracle, torch_dev, depth, w, cls):
    from gpu_stages import run_stages
    n1, n2, P = _case(mp, depth, w, cls)
    _split_instance(mp, n1, n2, depth, w)
    NC, bits1 = P["NC"], P["bits1"]
    a = _last_row_ones(mp, n1, P["j1"], NC, bits1, 0x5111 + 31 * depth + n1 % 977)
    b = _last_row_ones(mp, n2, P["j2"], NC, bits1, 0x5222 + 17 * w + n2 % 977)
    got = mp.mul(a, b, depth, w)
    assert (got == oracle.gmp_mul(a, b)).all(), f"{cls}: product differs (last row all-ones)"
    a1 = np.full(n1, ONES, dtype=np.uint64)
    b1 = np.full(n2, ONES, dtype=np.uint64)
    got = mp.mul(a1, b1, depth, w)
    assert (got == oracle.gmp_mul(a1, b1)).all(), f"{cls}: product differs (all-ones)"
    N = (1 << depth) * w
    if float(P["trunc"]) * N * N <= STAGE_COST_MAX:
        fails = run_stages(mp, depth, w, a, b, dev=torch_dev, check=("fwd", "inv", "comb"), mul=oracle.gmp_mul)
        assert not fails, "\n".join(fails[:5])


def test_mul6_unchanged(mp, oracle):
    """the sqrt2 front end splits in its own kernel and hands k_rpass no operand pointers: its
    forward columns keep the full bounds (second half: every row live)"""
    from helpers import max_limbs6
    depth, w = 6, 1024
    m = (3 * max_limbs6(depth, w)) // 4
    a = mp.fill_random(m, 0x6161)
    b = mp.fill_random(m - 5, 0x6262)
    b[-40:] = ONES
    r = mp.mul6(a, b, depth, w)
    assert (r == oracle.new_mpn_mul6(a, b, depth, w)).all()
    assert to_int(r) == to_int(a) * to_int(b)
