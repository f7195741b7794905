"""CPU tests of the shape sweeps (tests/sweep_shapes.py): every enumerated shape is valid, the counts
are pinned (a sweep that silently shrinks fails here, not on the GPU), the grids reach at least 100
distinct plans each, and the curated tables of the per-family GPU modules reach under 15 % of them --
the gap the sweeps close.  The reference's folding is checked against % on small shapes."""
import random

import pytest

import stage_model as sm
import sweep_shapes as ss
from helpers import to_int

MOD_BY_DEPTH = {2: 14, 3: 16, 4: 18, 5: 18, 6: 17, 7: 13, 8: 9, 9: 4, 10: 1}
MUL_BY_DEPTH = {2: 14, 3: 16, 4: 18, 5: 19, 6: 19, 7: 15, 8: 11, 9: 7, 10: 2}   # K = 1, 2 and 3 alike
MUL_FAMILIES = {1: ("mul", "sqr"), 2: ("dot2",), 3: ("dot3",)}


def _check(mp, family):
    return getattr(mp, family + "_check_params")


@pytest.mark.parametrize("family", ss.MOD_FAMILIES)
def test_mod_shapes_are_valid_and_counted(mp, family):
    grid = ss.mod_grid(family)
    assert sum(MOD_BY_DEPTH.values()) == 110
    assert {d: len(v) for d, v in ss.by_depth(grid).items()} == MOD_BY_DEPTH
    deep, edges = ss.mod_deep(family), ss.mod_edges(family)
    assert len(deep) == 16 and {s[2] for s in deep} == {18944}
    assert len(edges) == (13 if family == "mulmodw" else 12)
    for depth, w, L in grid + deep + edges:
        assert _check(mp, family)(L, depth, w) == 0, (family, depth, w, L)
    for depth, w, L in grid:   # the largest L: the next multiple of 64 bits is refused
        P = getattr(mp, family + "_plan_info")(L, depth, w)
        assert P["bits1"] * 2 * P["n"] == 64 * L and P["l"] <= ss.MAX_L
        step = 1
        while (2 * P["n"] * step) % 64:
            step += 1
        assert _check(mp, family)(2 * P["n"] * (P["bits1"] + step) // 64, depth, w) != 0, (family, depth, w, L)
    b1 = sorted(getattr(mp, family + "_plan_info")(L, depth, w)["bits1"] for depth, w, L in deep)
    assert (b1[0], b1[-1]) == (37, 296)
    assert max(getattr(mp, family + "_plan_info")(L, depth, w)["NC"] for depth, w, L in deep) == 128
    assert max(getattr(mp, family + "_plan_info")(L, depth, w)["NR"] for depth, w, L in deep) == 256


def test_mod_edges_sit_on_the_chain_blocks(mp):
    """k_nwrap / k_nwrapw: 1024-limb blocks, k_cwrap: 2048-limb blocks; pieces of 1, 2, 3 bits"""
    for family, block in (("mulmod", 1024), ("mulmodw", 1024), ("mulmodm1", 2048)):
        Ls = {L for _, _, L in ss.mod_edges(family)}
        for k in (1, 2, 3):
            assert {k * block - 1, k * block, k * block + 1} <= Ls, (family, k)
        sk = getattr(mp, family + "_stage_kernels")(block, 5, block // 8)
        assert ("k_cwrap" if family == "mulmodm1" else "k_nwrapw" if family == "mulmodw" else "k_nwrap") in sk["combine"], sk
    for family in ("mulmod", "mulmodm1"):
        assert [getattr(mp, family + "_plan_info")(L, 5, 4096)["bits1"] for L in (1, 2, 3)] == [1, 2, 3]
    assert mp.mulmodw_plan_info(32, 5, 64)["bits1"] == 32 and mp.mulmodw_check_params(31, 5, 64) != 0


@pytest.mark.parametrize("K", [1, 2, 3])
def test_mul_shapes_are_valid_and_counted(mp, K):
    grid = ss.mul_grid(K)
    assert {d: len(v) for d, v in ss.by_depth(grid).items()} == MUL_BY_DEPTH
    for depth, w, n in grid:
        assert mp.dot_check_params(K, n, n, depth, w) == 0
        assert mp.dot_check_params(K, n + 1, n + 1, depth, w) != 0, (K, depth, w, n)   # the largest n
        if K == 1:
            assert mp.check_params(n, n, depth, w) == 0
        else:
            assert n == mp.dot_max_limbs(K, depth, w)
            assert mp.sdot_check_params(K, 1, n, n, depth, w) == 0


def _grids(mp):
    out = [(f, ss.mod_grid(f)) for f in ss.MOD_FAMILIES]
    for K, fams in MUL_FAMILIES.items():
        out += [(f, ss.mul_grid(K)) for f in fams]
    return out


def test_every_grid_reaches_a_hundred_plans(mp):
    for family, grid in _grids(mp):
        assert len({ss.signature(mp, family, s) for s in grid}) >= 100, family
        assert sum(s[1] % 2 for s in grid) >= 12, family
        assert sum(s[1] & (s[1] - 1) != 0 for s in grid) >= 45, family


def _curated():
    """family -> the (depth, w, size or None) of the curated tables, imported from their modules;
    rows under an MPFFT_POINTWISE override are left out (the sweeps run the planner's own choice)"""
    import test_gpu_mulmod
    import test_gpu_mulmodm1
    import test_gpu_mulmodw
    import test_gpu_sdot
    import test_gpu_sqr
    plain = [s[:3] for s in test_gpu_sqr.WHOLE if s[3] is None]
    sums = plain + [s[:3] for s in test_gpu_sdot.SHAPES if s[3] is None]
    return {"mulmod": [s[:3] for s in test_gpu_mulmod.WHOLE], "mulmodm1": [s[:3] for s in test_gpu_mulmodm1.WHOLE],
            "mulmodw": [s[:3] for s in test_gpu_mulmodw.WHOLE], "mul": plain, "sqr": plain, "dot2": sums, "dot3": sums}


def test_the_curated_tables_reach_under_15_percent(mp):
    curated = _curated()
    for family, grid in _grids(mp):
        K = int(family[3:]) if family.startswith("dot") else 1
        have = set()
        for depth, w, n in curated[family]:
            if n is None:
                n = ss.mul_limbs(K, depth, w)
            if family.startswith("dot"):
                n = min(n, ss.mul_limbs(K, depth, w))   # as test_whole_signed_sums does at K = 3
            have.add(ss.signature(mp, family, (depth, w, n)))
        sweep = {ss.signature(mp, family, s) for s in grid}
        assert len(curated[family]) >= 9
        assert len(sweep & have) < 0.15 * len(sweep), (family, len(sweep & have), len(sweep))


@pytest.mark.parametrize("family", ss.MOD_FAMILIES)
def test_folding_equals_the_remainder(family):
    """the GPU sweeps fold the full product at 2^B == -+1 (a % of that size costs seconds a shape):
    folding == % on three shapes per family, on random values and the ends of the range"""
    from test_gpu_mulmodm1 import modm1
    rng = random.Random(0xf01d)
    shapes = [ss.mod_grid(family)[i] for i in (0, 40, 70)] + ss.mod_edges(family)[:1]
    assert len({s[0] for s in shapes}) >= 3
    for depth, w, L in shapes:
        B = 64 * L
        M = (1 << B) + (-1 if family == "mulmodm1" else 1)
        for v in (rng.getrandbits(2 * B), 0, M - 1, M, M + 1, (M - 1) ** 2, M * (M - 1), (1 << (2 * B)) - 1, to_int([1] * L) ** 2):
            got = modm1(v, B) if family == "mulmodm1" else sm.modp(v, B)
            assert got == v % M, (family, depth, w, L)
