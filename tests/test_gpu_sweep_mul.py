"""GPU sweep of the square, the cached operand, the sums and the signed sums of products over every
(depth, w) of tests/sweep_shapes.py at its largest balanced size up to 20 000 limbs (121 plans per
entry, against the nine to sixteen of the curated tables), and unbalanced operands at one (depth, w)
per depth.

Every call runs on a workspace of 0xFF bytes and writes d_r between poisoned guard limbs.  The
reference is GMP products (oracle.gmp_mul) added and subtracted as Python integers; bit-exact is the
only bar, and an enumerated shape the library refuses is a failure."""
import numpy as np
import pytest

import sweep_shapes as ss
from helpers import from_int, to_int
from test_gpu_dot import _ones_product, _t
from test_gpu_sdot import torch_dev   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

ONES = 2**64 - 1
ENTRY_K = {"sqr": 1, "precomp": 1, "dot2": 2, "dot3": 3, "sdot2": 2, "sdot3": 3}
MASKS = {"sdot2": (0b01, 0b10, 0b11), "sdot3": (0b101,)}
CASES = [(e, d) for e, K in ENTRY_K.items() for d in sorted(ss.by_depth(ss.mul_grid(K)))]


def _sync():
    import torch
    torch.cuda.synchronize()


def _mul(mp, dev, a, b, depth, w):
    n1, n2 = len(a), len(b)
    ws = mp.alloc_workspace(n1, n2, depth, w, dev)
    ws.fill_(0xFF)
    dr = ss.Guarded(dev, n1 + n2)
    mp.mul_device(dr.t, _t(a, dev), n1, _t(b, dev), n2, depth, w, ws)
    _sync()
    assert dr.intact()
    return dr.host()


def _sqr(mp, oracle, dev, depth, w, n):
    ws = mp.alloc_workspace_sqr(n, depth, w, dev)
    for name, a in (("random", mp.fill_random(n, 0x5a00 + 31 * depth + w)), ("all-ones", np.full(n, ONES, np.uint64))):
        ws.fill_(0xFF)
        dr = ss.Guarded(dev, 2 * n)
        mp.sqr_device(dr.t, _t(a, dev), n, depth, w, ws)
        _sync()
        assert dr.intact(), (depth, w, n, name)
        want = _ones_product(n, n) if name == "all-ones" else to_int(oracle.gmp_mul(a, a))
        assert to_int(dr.host()) == want, (depth, w, n, name)


def _precomp(mp, oracle, dev, depth, w, n1, n2):
    """one cache of b, two different a: limb-equal to mul_device and exact"""
    b = mp.fill_random(n2, 0x5b00 + 31 * depth + w)
    wsm = mp.alloc_workspace(n1, n2, depth, w, dev)
    wsp = mp.alloc_workspace_mul_precomp(n1, n2, depth, w, dev)
    pre = mp.alloc_precomp(n1, n2, depth, w, dev)
    wsm.fill_(0xFF)
    pre.fill_(0x5A)
    mp.precomp_device(pre, _t(b, dev), n1, n2, depth, w, wsm)
    _sync()
    snap = pre.clone()
    for k, a in enumerate((mp.fill_random(n1, 0x5c00 + depth + w), np.full(n1, ONES, np.uint64))):
        wsp.fill_(0xFF)
        dr = ss.Guarded(dev, n1 + n2)
        mp.mul_precomp_device(dr.t, _t(a, dev), n1, pre, n2, depth, w, wsp)
        _sync()
        assert dr.intact(), (depth, w, n1, n2, k)
        got = dr.host()
        assert (got == _mul(mp, dev, a, b, depth, w)).all(), (depth, w, n1, n2, k)
        assert (got == oracle.gmp_mul(a, b)).all(), (depth, w, n1, n2, k)
    assert bool((pre == snap).all()), "a multiply wrote to the cache"


class _Terms:
    """K random pairs and the all-ones pair on the device, their exact products computed once"""

    def __init__(self, mp, oracle, dev, K, n1, n2, seed):
        self.n1, self.n2 = n1, n2
        ha = [mp.fill_random(n1, seed + i) for i in range(K)]
        hb = [mp.fill_random(n2, seed + 16 + i) for i in range(K)]
        self.random = [(_t(a, dev), _t(b, dev)) for a, b in zip(ha, hb)]
        self.random_products = [to_int(oracle.gmp_mul(a, b)) for a, b in zip(ha, hb)]
        ones = (_t(np.full(n1, ONES, np.uint64), dev), _t(np.full(n2, ONES, np.uint64), dev))
        self.ones = [ones] * K
        self.ones_products = [_ones_product(n1, n2)] * K
        self.zero = _t(np.zeros(n1, np.uint64), dev)


def _dot(mp, dev, T, K, depth, w, sets=("random", "all-ones")):
    n1, n2 = T.n1, T.n2
    assert mp.dot_check_params(K, n1, n2, depth, w) == 0, (K, depth, w, n1, n2)
    ws = mp.alloc_workspace_dot(K, n1, n2, depth, w, dev)
    for name in sets:
        terms, prods = (T.random, T.random_products) if name == "random" else (T.ones, T.ones_products)
        ws.fill_(0xFF)
        dr = ss.Guarded(dev, n1 + n2 + 1)
        mp.dot_device(dr.t, [a for a, _ in terms], [b for _, b in terms], n1, n2, depth, w, ws)
        _sync()
        assert dr.intact(), (K, depth, w, n1, n2, name)
        assert (dr.host() == from_int(sum(prods), n1 + n2 + 1)).all(), (K, depth, w, n1, n2, name)


def _sdot(mp, dev, T, K, masks, depth, w, sets=("random", "all-ones", "a b - a b")):
    n1, n2 = T.n1, T.n2
    nl = n1 + n2 + 1
    ws = mp.alloc_workspace_sdot(K, n1, n2, depth, w, dev)
    for neg in masks:
        assert mp.sdot_check_params(K, neg, n1, n2, depth, w) == 0, (K, neg, depth, w, n1, n2)
        sign = [-1 if (neg >> i) & 1 else 1 for i in range(K)]
        for name in sets:
            if name == "a b - a b":   # the exact cancellation: one product under both signs, any other term 0 b
                if len(set(sign)) == 1:
                    continue
                keep = (sign.index(1), sign.index(-1))
                terms = [T.random[0] if i in keep else (T.zero, T.random[0][1]) for i in range(K)]
                prods = [T.random_products[0] if i in keep else 0 for i in range(K)]
            else:
                terms, prods = (T.random, T.random_products) if name == "random" else (T.ones, T.ones_products)
            ws.fill_(0xFF)
            dr = ss.Guarded(dev, nl)
            mp.sdot_device(dr.t, [a for a, _ in terms], [b for _, b in terms], neg, n1, n2, depth, w, ws)
            _sync()
            assert dr.intact(), (K, bin(neg), depth, w, n1, n2, name)
            val = sum(s * p for s, p in zip(sign, prods))
            got = dr.host()
            assert (got == from_int(val % (1 << (64 * nl)), nl)).all(), (K, bin(neg), depth, w, n1, n2, name)
            assert mp.sdot_to_int(got) == val
            if name == "a b - a b":
                assert val == 0 and not got.any()


@pytest.mark.parametrize("entry,depth", CASES, ids=["%s-d%d" % c for c in CASES])
def test_every_plan_of_the_grid(mp, oracle, torch_dev, entry, depth):
    K = ENTRY_K[entry]
    shapes = ss.by_depth(ss.mul_grid(K))[depth]
    assert 1 <= len(shapes) <= 19
    for d, w, n in shapes:
        assert n == ss.mul_limbs(K, d, w)
        if entry == "sqr":
            assert mp.check_params(n, n, d, w) == 0
            _sqr(mp, oracle, torch_dev, d, w, n)
        elif entry == "precomp":
            assert mp.check_params(n, n, d, w) == 0
            _precomp(mp, oracle, torch_dev, d, w, n, n)
        else:
            T = _Terms(mp, oracle, torch_dev, K, n, n, 0x5d00 + 31 * d + w)
            if entry.startswith("dot"):
                _dot(mp, torch_dev, T, K, d, w)
            else:
                _sdot(mp, torch_dev, T, K, MASKS[entry], d, w)


def _largest_n1(mp, K, depth, w, n2_of, cap=20000):
    """the largest n1 <= cap the K-term sum accepts with n2 = n2_of(n1)"""
    ok = lambda n1: n2_of(n1) >= 1 and mp.dot_check_params(K, n1, n2_of(n1), depth, w) == 0
    lo, hi = 0, cap
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


UNBALANCED = [v[len(v) // 2][:2] for _, v in sorted(ss.by_depth(ss.mul_grid(3)).items())]


@pytest.mark.parametrize("depth,w", UNBALANCED, ids=["d%d-w%d" % s for s in UNBALANCED])
def test_unbalanced_operands(mp, oracle, torch_dev, depth, w):
    """n2 = 1 and n2 = n1 / 5 with n1 as large as the sum of three admits, both ways round: the
    multiply against the cached operand, the sum of two and of three, the signed sum of three"""
    K = 3
    for n2_of in (lambda n1: 1, lambda n1: n1 // 5):
        n1 = _largest_n1(mp, K, depth, w, n2_of)
        n2 = n2_of(n1)
        assert n1 >= 5 and mp.dot_check_params(K, n1, n2, depth, w) == 0, (depth, w, n1, n2)
        assert n1 == 20000 or mp.dot_check_params(K, n1 + 1, n2_of(n1 + 1), depth, w) != 0
        for m1, m2 in ((n1, n2), (n2, n1)):
            assert mp.dot_check_params(K, m1, m2, depth, w) == 0, (depth, w, m1, m2)
            _precomp(mp, oracle, torch_dev, depth, w, m1, m2)
            T = _Terms(mp, oracle, torch_dev, K, m1, m2, 0x5e00 + 31 * depth + w)
            _dot(mp, torch_dev, T, K, depth, w)
            _sdot(mp, torch_dev, T, K, (0b101,), depth, w)
            T2 = _Terms(mp, oracle, torch_dev, 2, m1, m2, 0x5f00 + 31 * depth + w)
            _dot(mp, torch_dev, T2, 2, depth, w, sets=("random",))
