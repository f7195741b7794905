"""GPU sweep of the products mod 2^B + 1, mod 2^B - 1 and mod 2^B + 1 with the low-word CRT over
every (depth, w) of tests/sweep_shapes.py at its largest L up to 20 000 limbs (110 plans a family,
against the dozen of each family's curated table), the deep plans (depth 11..14) and the result
lengths on the block edges of the chains that end the products, with the combine stage alone on
placed coefficients there.

Every call runs on a workspace of 0xFF bytes and writes d_r between poisoned guard limbs.  The
reference is GMP (oracle.gmp_mul) folded at 2^B == -+1 (stage_model.modp, modm1) or Python integers;
bit-exact is the only bar, and an enumerated shape the library refuses is a failure."""
import random

import numpy as np
import pytest

import stage_model as sm
import sweep_shapes as ss
import test_gpu_mulmod as tm
import test_gpu_mulmodm1 as tc
import test_gpu_mulmodw as tw
from helpers import from_int, to_int
from test_gpu_sdot import torch_dev   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

MODULE = {"mulmod": tm, "mulmodm1": tc, "mulmodw": tw}
# the operands the square runs on: random, the largest reduced value below the wrap, M - 1
SQUARED = {"mulmod": ("random", "2^B-1 squared", "2^B squared"), "mulmodw": ("random", "2^B-1 squared", "2^B squared"),
           "mulmodm1": ("random", "all-ones squared", "M-1 squared")}
NEEDED = {"mulmod": {"random", "2^B-1 squared", "2^B squared", "2 times 2^(B-1)", "one", "zero", "top pieces"},
          "mulmodm1": {"random", "all-ones squared", "M-1 squared", "2 times 2^(B-1)", "one", "zero", "top pieces"}}
NEEDED["mulmodw"] = NEEDED["mulmod"]
CASES = [(f, d) for f in ss.MOD_FAMILIES for d in sorted(ss.by_depth(ss.mod_grid(f)))]


def _rlen(family, L):
    return L if family == "mulmodm1" else L + 1


def _workspace(mp, family, L, depth, w, sqr, dev):
    if family == "mulmodm1":
        return mp.alloc_workspace_mulmodm1(L, depth, w, 1 if sqr else 0, dev)
    return getattr(mp, "alloc_workspace_" + family)(L, depth, w, sqr, dev)


def _run(mp, dev, family, a, b, depth, w, L, ws):
    """the device product (b None: the square) on a 0xFF workspace, d_r between guards"""
    import torch
    stem = family[3:]   # mod, modm1, modw
    dr = ss.Guarded(dev, _rlen(family, L))
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    ws.fill_(0xFF)
    if b is None:
        getattr(mp, "sqr" + stem + "_device")(dr.t, da, L, depth, w, ws)
    else:
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        getattr(mp, "mul" + stem + "_device")(dr.t, da, db, L, depth, w, ws)
    torch.cuda.synchronize()
    assert dr.intact(), (family, depth, w, L, "wrote outside d_r")
    return dr.host()


def _reduced(family, got, L):
    if family == "mulmodm1":
        return not (got == 2**64 - 1).all()
    return got[L] == 0 or (got[L] == 1 and not got[:L].any())


def _expected(family, oracle, a, b, L):
    full = to_int(oracle.gmp_mul(a, b))
    return tc.modm1(full, 64 * L) if family == "mulmodm1" else sm.modp(full, 64 * L)


def _sweep_one(mp, oracle, dev, family, depth, w, L):
    assert getattr(mp, family + "_check_params")(L, depth, w) == 0, (family, depth, w, L)
    ops = [(o[0], o[1], o[2]) for o in MODULE[family]._operands(mp, depth, w, L, 0x5e00 + 131 * depth + w)]
    assert NEEDED[family] <= {name for name, _, _ in ops}
    other = {"mulmod": "mulmodw", "mulmodw": "mulmod"}.get(family)
    both = other is not None and getattr(mp, other + "_check_params")(L, depth, w) == 0
    ws = _workspace(mp, family, L, depth, w, False, dev)
    wsq = _workspace(mp, family, L, depth, w, True, dev)
    wso = _workspace(mp, other, L, depth, w, False, dev) if both else None
    for name, a, b in ops:
        tag = (family, depth, w, L, name)
        got = _run(mp, dev, family, a, b, depth, w, L, ws)
        assert _reduced(family, got, L), tag
        assert to_int(got) == _expected(family, oracle, a, b, L), tag
        if both:
            assert (_run(mp, dev, other, a, b, depth, w, L, wso) == got).all(), tag
        if name in SQUARED[family]:
            mu = got if b is a or (a == b).all() else _run(mp, dev, family, a, a, depth, w, L, ws)
            sq = _run(mp, dev, family, a, None, depth, w, L, wsq)
            assert (sq == mu).all(), tag
            assert _reduced(family, sq, L) and to_int(sq) == _expected(family, oracle, a, a, L), tag
    return both


@pytest.mark.parametrize("family,depth", CASES, ids=["%s-d%d" % c for c in CASES])
def test_every_plan_of_the_grid(mp, oracle, torch_dev, family, depth):
    shapes = ss.by_depth(ss.mod_grid(family))[depth]
    assert 1 <= len(shapes) <= 18
    both = sum(_sweep_one(mp, oracle, torch_dev, family, d, w, L) for d, w, L in shapes)
    if family == "mulmod" and depth >= 4:
        assert both >= 1   # the plain family's full sizes with bits1 >= 32 are valid with the CRT too


@pytest.mark.parametrize("family", ss.MOD_FAMILIES)
@pytest.mark.parametrize("depth", [11, 12, 13, 14])
def test_deep_plans(mp, oracle, torch_dev, family, depth):
    """depth 11..14 at w = 1, 2, 3, 4: several column and row passes on small coefficients"""
    shapes = ss.by_depth(ss.mod_deep(family))[depth]
    assert len(shapes) == 4
    for d, w, L in shapes:
        _sweep_one(mp, oracle, torch_dev, family, d, w, L)


EDGES = [(f,) + s for f in ss.MOD_FAMILIES for s in ss.mod_edges(f)]
EDGE_IDS = ["%s-d%d-w%d-L%d" % e for e in EDGES]


@pytest.mark.parametrize("family,depth,w,L", EDGES, ids=EDGE_IDS)
def test_block_edges_and_short_pieces(mp, oracle, torch_dev, family, depth, w, L):
    _sweep_one(mp, oracle, torch_dev, family, depth, w, L)


def _place_canonical(mp, dev, family, ws, L, depth, w, cs, N, l):
    """c_j mod p as canonical residues into operand A's slots (and c_j mod 2^32 into d with the CRT)"""
    import torch
    p = (1 << N) + 1
    if family == "mulmodm1":
        tc._place(mp, dev, ws, L, depth, w, [(from_int(c, l), (), (), 0) for c in cs])
        return
    enc = [(from_int((c % p) & ((1 << N) - 1), l), (), (), (c % p) >> N) for c in cs]
    if family == "mulmod":
        tm._place(mp, dev, ws, L, depth, w, enc)
        return
    dig, top, cb, d = mp.mulmodw_workspace_views(ws, L, depth, w)
    dig.copy_(torch.from_numpy(np.stack([e[0] for e in enc]).view(np.int64)).to(dev))
    top.copy_(torch.from_numpy(np.array([e[3] for e in enc], dtype=np.int32)).to(dev))
    cb.zero_()
    d.copy_(torch.from_numpy(np.array([c % (1 << 32) for c in cs], dtype=np.uint32).view(np.int32)).to(dev))


@pytest.mark.parametrize("family,depth,w,L", EDGES, ids=EDGE_IDS)
def test_combine_stage_at_the_block_edges(mp, torch_dev, family, depth, w, L):
    """MPFFT_STAGE_COMBINE on placed canonical coefficients at the edge lengths: each family's own
    patterns (a carry or borrow through every limb, an end-around carry past all-ones limbs), the
    flags and scratch starting as 0x5A bytes, d_r between guards"""
    import torch
    P = getattr(mp, family + "_plan_info")(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N, B = P["n"] * w, 64 * L
    rng = random.Random(0xed9e + L)
    if family == "mulmod":
        pats = [(name, cs) for name, cs in tm._combine_patterns(n2, b1, depth, B, rng)]
    elif family == "mulmodm1":
        pats = [(name, cs) for name, cs, _ in tc._combine_patterns(n2, b1, depth, N, B, rng, False)]
    else:
        pats = tw._combine_patterns(n2, b1, N, rng)
    assert len(pats) >= 10
    ws = _workspace(mp, family, L, depth, w, False, torch_dev)
    for name, cs in pats:
        ws.fill_(0x5A)
        dr = ss.Guarded(torch_dev, _rlen(family, L))
        _place_canonical(mp, torch_dev, family, ws, L, depth, w, cs, N, l)
        getattr(mp, family + "_stage")(mp.STAGE_COMBINE, dr.t, dr.t, dr.t, L, depth, w, ws)
        torch.cuda.synchronize()
        total = sum(c << (j * b1) for j, c in enumerate(cs))
        want = tc.modm1(total, B) if family == "mulmodm1" else sm.modp(total, B)
        got = dr.host()
        assert dr.intact(), (family, depth, w, L, name)
        assert _reduced(family, got, L) and to_int(got) == want, (family, depth, w, L, name)
