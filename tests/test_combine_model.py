"""CPU checks of tests/combine_model.py, the exact model the placed combine tests compare the GPU
against (tests/test_gpu_combine_placed.py): the closed form of a stripe's phase-0 value against the
limb-by-limb chain, the chained stripes against the plain sum on the planner's real partitions, and
the properties that make each pattern worth running -- so that a planner change cannot quietly
empty the GPU test."""
import pytest

import combine_model as cm

SW = pytest.mark.parametrize("shape,world", cm.SHAPE_WORLDS, ids=[f"{s[0]}-{s[1]}-{s[2]}-w{w}" for s, w in cm.SHAPE_WORLDS])


def _contract(mp, shape, world):
    depth, w, n1, n2 = shape
    return cm.shard_contract(mp, n1, n2, depth, w, world)


@pytest.mark.parametrize("shape,worlds", [(s, ws) for s, ws, _, _ in cm.SHAPES[:2]], ids=["l1", "l4"])
def test_closed_form_against_per_limb_chain(mp, shape, worlds):
    """every stripe of every pattern on the two smallest shapes: the windowed sum, the A(m) form
    and the naive per-limb loop give the same (limbs, generate, propagate)"""
    for world in worlds:
        K = _contract(mp, shape, world)
        for name, c in cm.cases(K, 11 + world):
            for s in range(K.S):
                want = cm.stripe_naive(K, c, s)
                assert cm.stripe_value(K, c, s) == want, (world, name, s)
                assert cm.stripe_value_A(K, c, s) == want, (world, name, s)


def test_single_stripe_is_the_plain_sum(mp):
    """one stripe over the whole product (the single-GPU combine): phase 0 is already the sum"""
    depth, w, n1, n2 = cm.SHAPES[1][0]
    P = mp.plan_info(n1, n2, depth, w)
    K = cm.single_contract(P["n"] * w, P["bits1"], P["j1"] + P["j2"] - 1, n1 + n2)
    for name, c in cm.cases(K, 5, halo=False):
        x, g, p = cm.stripe_value(K, c, 0)
        assert x == cm.product(K, c), name


@SW
def test_chained_stripes_give_the_product(mp, shape, world):
    """phase 0, the (generate, propagate) chain and phase 1 reproduce sum c_k 2^(k bits1) mod
    2^(64 total) for every pattern; and what each pattern is there for holds on this partition"""
    K = _contract(mp, shape, world)
    allcases = cm.cases(K, 1)
    names = [n for n, _ in allcases]
    assert len(set(names)) == len(names)
    for name, c in allcases:
        st = cm.phase0(K, c)
        assert cm.assemble(K, cm.phase1(K, st)) == cm.product(K, c), name
        inf = cm.info(K, c)
        if name == "ripple":
            # one stripe generates: the first non-empty one, or the one after it where the carry leaves
            # that stripe as its last window sum's overflow
            gen = [i for i in inf if i["g"]]
            assert len(gen) == 1 and len([i for i in inf[:gen[0]["s"]] if i["n"]]) <= 1
            through = [i for i in inf if i["cin"] and i["p"] and i["n"]]
            assert through, "no wholly all-ones stripe takes the carry"
            if world > 1:   # the carry passes all-ones stripes of other ranks than the one generating it
                assert any(i["rank"] != gen[0]["rank"] for i in through)
                assert any(a["rank"] != b["rank"] for a, b in zip(through, through[1:]))
        elif name.startswith("stop "):
            s, off = (int(x) for x in name[6:].split("+"))
            # the carry enters the stripe as its carry-in and wraps `off` all-ones limbs (on the smallest
            # shape it can enter as the overflow of the window sum below the stripe instead)
            assert inf[s]["cin"] == 1 or off < 256, (name, inf[s])
            if inf[s]["cin"]:
                assert inf[s]["lead"] == off and not inf[s]["p"], (name, inf[s])
            assert all(i["cin"] == 0 for i in inf[s + 1:]), name
        elif name == "random":
            assert not any(i["g"] for i in inf), "a random product carried between stripes"
        elif name == "two ripples" and len([i for i in inf if i["n"]]) >= 6 and K.bits1 >= 64:
            gens = [i["s"] for i in inf if i["g"]]
            assert len(gens) >= 2, name
            # generate, then propagate, then a kill before the second generate
            assert any(i["cin"] and i["p"] and i["n"] for i in inf[:gens[1]])
            assert any(not i["cin"] for i in inf[gens[0] + 1: gens[1] + 1])
            assert any(i["cin"] and i["p"] and i["n"] for i in inf[gens[1] + 1:])
        elif name == "max" and K.S > 1:   # an overflow of a window sum is handed across a stripe boundary
            assert any(cm.window_sum(K, c, K.ms[s] - 1)[1] for s in range(1, K.S) if K.n(s))
    # the chunk edges of k_stripe_carry are reached wherever a stripe is long enough for them
    for s in cm.stop_stripes(K):
        for off in (256, 257):
            if off < K.n(s) and cm.stop_bit(K, K.ms[s] + off) is not None:
                assert f"stop s{s}+{off}" in names
    longest = max(K.n(s) for s in cm.stop_stripes(K))
    if longest > 257:
        assert any(n.endswith("+256") for n in names) and any(n.endswith("+257") for n in names)
    halos = [n for n in names if n.startswith("halo s")]
    assert len(halos) >= min(K.H, K.len - 1) if K.S > 1 else True


def test_shape_table_facts(mp):
    """the (shape, world, form) table of the GPU test against the planner: l, the k_combine1 form,
    halos longer than a stripe, empty stripes, several blocks per stripe, more than 256 stripes"""
    for shape, world in cm.SHAPE_WORLDS:
        cm.check_shape_facts(_contract(mp, shape, world), shape, world)


def test_whole_path_operands_carry_through_other_ranks(mp):
    """the operands of the whole-path GPU case: their coefficients send a carry-in of 1 through at
    least 300 all-ones limbs of wholly all-ones stripes on different ranks"""
    depth, w, n1, n2 = cm.WHOLE_PATH[0]
    K = cm.shard_contract(mp, n1, n2, depth, w, cm.WHOLE_PATH[1])
    a, b = cm.carry_operands(K)
    c = cm.convolution(K, a, b)
    cm.check_range(K, c)
    assert cm.product(K, c) == a * b
    inf = cm.info(K, c)
    run = best = 0
    ranks = set()
    for i in inf:
        if i["cin"] and i["p"] and i["n"]:
            run += i["n"]
            ranks.add(i["rank"])
            best = max(best, run if len(ranks) > 1 else 0)
        else:
            run, ranks = 0, set()
    assert best >= 300
