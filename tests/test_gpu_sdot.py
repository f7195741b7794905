"""GPU tests of the signed sums of products (mpfft_sdot_*): r = sum_i +-a_i b_i in two's complement,
K forward transform pairs and one inverse.

Whole signed sums through every pointwise family and combine path, exact cancellations and long
borrows, neg == 0 against dot_device, K = 1 against the negated multiply, the accumulator D at its
extreme (64 all-ones terms), unbalanced operands, the correction alone on hand-filled d_r at every
size around the chain block, the stages composed by hand, the workspace guard, back-to-back sums,
the host entries, profiling and a plain C caller.  The reference is Python integers and GMP products
(oracle.gmp_mul); bit-exact is the only bar.  Every case asserts its kernel class through
sdot_stage_kernels first."""
import ctypes
import math
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import from_int, to_int
from test_gpu_dot import _Pool, _check_class, _ones_product, _t, torch_dev   # noqa: F401 (torch_dev: a fixture)
from test_gpu_sqr import PAIR, QUAD, FOLD, _pointwise_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENOMEM = 4
SDNEG = "k_sdneg + "
SDFIX = " + k_sdedge + k_sdfix (blocks of 4096 limbs)"
ONES = 2**64 - 1


def _check_sclass(mp, K, neg, n1, n2, depth, w, head, has=None, scale=None, combine=None):
    """the dot's class (_check_class), and the two fields a negative term changes"""
    dot = _check_class(mp, K, n1, n2, depth, w, head, has, scale, combine)
    sk = mp.sdot_stage_kernels(K, neg, n1, n2, depth, w)
    assert sk["fwd_columns"] == (SDNEG if neg else "") + dot["fwd_columns"], sk
    assert sk["combine"] == dot["combine"] + (SDFIX if neg else ""), sk
    assert all(sk[k] == dot[k] for k in mp.STAGE_NAMES if k not in ("fwd_columns", "combine")), sk
    assert mp.SDOT_FIX_BLOCK == 4096   # the chain block the sizes below are placed around
    return sk


def _sdot(mp, dev, terms, neg, n1, n2, depth, w, ws=None):
    """terms: (a tensor, b tensor) per term; the n1 + n2 + 1 limbs of the signed sum"""
    import torch
    K = len(terms)
    dr = torch.full((n1 + n2 + 1,), 0x5a5a5a5a, dtype=torch.int64, device=dev)
    if ws is None:
        ws = mp.alloc_workspace_sdot(K, n1, n2, depth, w, dev)
    mp.sdot_device(dr, [a for a, _ in terms], [b for _, b in terms], neg, n1, n2, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _twos(x, nl):
    return from_int(x % (1 << (64 * nl)), nl)


class _SPool(_Pool):
    """_Pool with a zero b, unit operands, and signed sums"""

    def __init__(self, mp, oracle, dev, n1, n2, seed):
        super().__init__(mp, oracle, dev, n1, n2, seed)
        ua, ub = np.zeros(n1, np.uint64), np.zeros(n2, np.uint64)
        ua[0] = ub[0] = 1
        for k, v in (("0b", np.zeros(n2, np.uint64)), ("ua", ua), ("ub", ub)):
            self.h[k] = v
            self.d[k] = _t(v, dev)

    def product(self, x, y):
        if (x, y) not in self.prod and (x[0] in "0u" or y[0] in "0u"):
            self.prod[(x, y)] = to_int(self.h[x]) * to_int(self.h[y])   # a zero or single-limb operand
        return to_int(self.want([(x, y)]))

    def signed(self, names, neg):
        tot = sum((-1 if (neg >> i) & 1 else 1) * self.product(x, y) for i, (x, y) in enumerate(names))
        return tot, _twos(tot, self.n1 + self.n2 + 1)


def _signed_sets(K, neg):
    """(label, term names) for mask neg: random operands, every operand all-ones, a zero a and a zero b
    in a negative term, a_i == b_i aliased in a negative term (n1 == n2), one pointer in a positive and
    a negative term (in two negative terms where none is positive)"""
    rnd = [("a0", "b0"), ("a1", "b1"), ("a2", "b2")][:K]
    ni = [i for i in range(K) if (neg >> i) & 1][0]
    pos = [i for i in range(K) if not (neg >> i) & 1]
    oi = pos[0] if pos else [i for i in range(K) if i != ni][0]

    def with_term(i, t):
        return rnd[:i] + [t] + rnd[i + 1:]
    shared = with_term(oi, (rnd[ni][0], rnd[oi][1]))
    return [("random", rnd), ("all-ones", [("1a", "1b")] * K),
            ("zero a, negative", with_term(ni, ("0a", rnd[ni][1]))), ("zero b, negative", with_term(ni, (rnd[ni][0], "0b"))),
            ("a == b, negative", with_term(ni, ("a0", "a0"))), ("shared pointer", shared)]


# (depth, w, n, MPFFT_POINTWISE, pointwise starts with, contains, scale, combine): one per pointwise
# family and combine path
SHAPES = [
    (7, 1024, 131064, None, "k_pwss<18>", (), "k_rscale", "k_combine1"),
    (5, 4096, 20000, None, "k_pwss<18>", (), "(folded", FOLD),
    (8, 512, 140000, None, "k_pwss<18>", (PAIR,), None, None),
    (14, 8, 500000, None, "k_pwss<18>", (QUAD,), None, None),
    (6, 1024, 32760, "pwss", "k_pwss<10>", (), None, None),
    (11, 8, 5000, None, "k_pwm2", (), None, None),
    (9, 16, None, None, "k_pwm ", (), None, None),
    (8, 8, None, None, "k_pw ", (), None, None),
    (9, 2, 120, None, "k_pointwise", (), None, None),
]


@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine", SHAPES)
def test_whole_signed_sums(mp, oracle, torch_dev, depth, w, n, kind, head, has, scale, combine):
    n_shape, pool = n, None
    with _pointwise_env(kind):
        for K, masks in ((2, (0b01, 0b10, 0b11)), (3, (0b010, 0b101))):
            # "max", and (7, 1024, 131064) at K = 3: the largest operands of this K (131062 limbs there)
            n = min(n_shape or 1 << 40, mp.dot_max_limbs(K, depth, w))
            assert n_shape in (None, 131064) or n == n_shape
            if pool is None or pool.n1 != n:
                pool = _SPool(mp, oracle, torch_dev, n, n, 0x5d07 + 31 * depth + w)
            assert mp.sdot_check_params(K, masks[0], n, n, depth, w) == 0, (K, depth, w, n)
            if depth == 8 and w == 512:
                P = mp.dot_plan_info(K, n, n, depth, w)
                assert P["trunc"] > P["n"]   # truncation case b
            ws = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)
            for neg in masks:
                _check_sclass(mp, K, neg, n, n, depth, w, head, has, scale, combine)
                for label, names in _signed_sets(K, neg):
                    got = _sdot(mp, torch_dev, pool.terms(names), neg, n, n, depth, w, ws)
                    val, want = pool.signed(names, neg)
                    assert (got == want).all(), (label, K, bin(neg), depth, w, n)
                    assert mp.sdot_to_int(got) == val
                    assert got[2 * n] < K or got[2 * n] >= 2**64 - K


def _unit(n, k, dev):
    e = np.zeros(n, np.uint64)
    e[k] = 1
    return _t(e, dev)


@pytest.mark.parametrize("depth,w,n1,n2,head", [(11, 8, 5000, 4000, "k_pwm2"), (9, 2, 120, 97, "k_pointwise")])
def test_cancellations_and_long_borrows(mp, oracle, torch_dev, depth, w, n1, n2, head):
    nl = n1 + n2 + 1
    pool = _SPool(mp, oracle, torch_dev, n1, n2, 0xca9 + depth)
    d = pool.d

    def run(terms, neg):
        _check_sclass(mp, len(terms), neg, n1, n2, depth, w, head)
        return _sdot(mp, torch_dev, terms, neg, n1, n2, depth, w)
    ab = (d["a0"], d["b0"])
    assert not run([ab, ab], 0b10).any()                                            # a b - a b = 0
    assert not run([ab, ab], 0b01).any()
    assert (run([(d["0a"], d["b1"]), (d["ua"], d["ub"])], 0b10) == ONES).all()        # 0 x - 1 1 = -1
    one = run([(d["ua"], d["ub"]), (d["0a"], d["b1"])], 0b10)                         # 1 1 - 0 x = 1
    assert one[0] == 1 and not one[1:].any()
    # a b + 2^(64 k) - a b and its negative: a borrow from limb k to the top, across every chain block
    # boundary above k; k at the boundary itself where the result spans one
    ks = [0, n1 - 1] + ([mp.SDOT_FIX_BLOCK - 1, mp.SDOT_FIX_BLOCK] if nl > mp.SDOT_FIX_BLOCK else [])
    assert nl <= mp.SDOT_FIX_BLOCK or nl > 2 * mp.SDOT_FIX_BLOCK
    for k in ks:
        ek = (_unit(n1, k, torch_dev), d["ub"])
        for terms, neg, val in (([ab, ek, ab], 0b100, 1 << (64 * k)), ([ab, ek, ab], 0b011, -(1 << (64 * k))),
                                ([ek, ab, ab], 0b101, -(1 << (64 * k))), ([ab, ab, ek], 0b010, 1 << (64 * k))):
            got = run(terms, neg)
            assert (got == _twos(val, nl)).all(), (k, bin(neg))


@pytest.mark.parametrize("depth,w,n,head", [(8, 512, 40000, "k_pwss<18>"), (9, 2, 120, "k_pointwise")])
def test_no_negative_term_is_dot_device(mp, torch_dev, depth, w, n, head):
    import torch
    K = 3
    _check_sclass(mp, K, 0, n, n, depth, w, head)
    terms = [(_t(mp.fill_random(n, 0x70 + i), torch_dev), _t(mp.fill_random(n, 0x80 + i), torch_dev)) for i in range(K)]
    dr = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
    mp.dot_device(dr, [a for a, _ in terms], [b for _, b in terms], n, n, depth, w, mp.alloc_workspace_dot(K, n, n, depth, w, torch_dev))
    torch.cuda.synchronize()
    ws = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)
    ws.fill_(0xC3)
    before = ws[mp.dot_workspace_bytes(K, n, n, depth, w):].clone()
    got = _sdot(mp, torch_dev, terms, 0, n, n, depth, w, ws)
    assert (got == dr.cpu().numpy().view(np.uint64)).all()
    assert torch.equal(ws[mp.dot_workspace_bytes(K, n, n, depth, w):], before)   # neither kernel ran


@pytest.mark.parametrize("depth,w,n,head", [(5, 4096, 20000, "k_pwss<18>"), (11, 8, 5000, "k_pwm2")])
def test_one_negative_term_is_the_negated_multiply(mp, torch_dev, depth, w, n, head):
    import torch
    _check_sclass(mp, 1, 1, n, n, depth, w, head)
    a, b = _t(mp.fill_random(n, 0x1a), torch_dev), _t(mp.fill_random(n, 0x1b), torch_dev)
    dm = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    mp.mul_device(dm, a, n, b, n, depth, w, mp.alloc_workspace(n, n, depth, w, torch_dev))
    torch.cuda.synchronize()
    got = _sdot(mp, torch_dev, [(a, b)], 1, n, n, depth, w)
    assert (got == _twos(-to_int(dm.cpu().numpy().view(np.uint64)), 2 * n + 1)).all()
    assert got[2 * n] == ONES


@pytest.mark.parametrize("npos", [0, 1])
def test_the_extreme_accumulator(mp, torch_dev, npos):
    """K = 64, all-ones operands at dot_max_limbs: 64 (63) operands of all-ones limbs summed into D --
    every overflow count at its largest -- and the tightest coefficients of the complemented terms"""
    depth, w, K = 9, 2, 64
    n = mp.dot_max_limbs(K, depth, w)
    neg = (1 << 64) - 1 if npos == 0 else ((1 << 64) - 1) & ~(1 << 17)
    _check_sclass(mp, K, neg, n, n, depth, w, "k_pointwise")
    ones = _t(np.full(n, ONES, np.uint64), torch_dev)
    got = _sdot(mp, torch_dev, [(ones, ones)] * K, neg, n, n, depth, w)
    assert mp.sdot_to_int(got) == -(64 - 2 * npos) * _ones_product(n, n)
    assert got[2 * n] == 2**64 - (64 - 2 * npos)


@pytest.mark.parametrize("depth,w,n1,n2,head", [(8, 512, 220000, 60000, "k_pwss<18>"), (8, 512, 60000, 220000, "k_pwss<18>"),
                                                (11, 8, 300, 5000, "k_pwm2"), (11, 8, 5000, 300, "k_pwm2"),
                                                (11, 8, 5000, 5000, "k_pwm2")])
def test_unbalanced_operands(mp, oracle, torch_dev, depth, w, n1, n2, head):
    """n1 >> n2: the + D and - (D << 64 n1) regions of the correction are disjoint; n1 << n2: they overlap"""
    K = 3
    pool = _SPool(mp, oracle, torch_dev, n1, n2, 0xb1 + depth + n1)
    ws = mp.alloc_workspace_sdot(K, n1, n2, depth, w, torch_dev)
    for neg in (0b101, 0b010):
        _check_sclass(mp, K, neg, n1, n2, depth, w, head)
        for names in ([("a0", "b0"), ("a1", "b1"), ("1a", "1b")], [("1a", "1b"), ("1a", "1b"), ("a2", "b2")]):
            got = _sdot(mp, torch_dev, pool.terms(names), neg, n1, n2, depth, w, ws)
            assert (got == pool.signed(names, neg)[1]).all(), (bin(neg), names)


# ---- the correction alone ---------------------------------------------------------------------------
B = 4096   # the chain block; asserted against the library's constant and kernel string in _check_sclass
FIX_SIZES = [(120, 97), (3000, B - 3001), (B - 3001, 3000), (5000, 2 * B - 5001), (2000, B - 2002), (2094, B - 2094),
             (4000, 2 * B - 4002), (4192, 2 * B - 4192), (300, 17000), (17000, 300), (9000, 9000)]


@pytest.mark.parametrize("n1,n2", FIX_SIZES)
def test_the_correction_alone(mp, torch_dev, n1, n2):
    """SD_NEG for j operands b (the later ones accumulating), d_r filled by hand, SD_FIX: against
    (r' - (2^(64 n1) - 1) sum b) mod 2^(64 (n1 + n2 + 1)) in Python integers, whatever D's form.
    Sizes n1 + n2 + 1: below a chain block, exactly one and two blocks, a limb less and a limb more,
    and more than four blocks."""
    import torch
    depth, w, K = 11, 8, 64
    nl = n1 + n2 + 1
    assert mp.SDOT_FIX_BLOCK == B and nl in (218, B, 2 * B, B - 1, B + 1, 2 * B - 1, 2 * B + 1, 17301, 18001)
    assert nl <= B or nl > 4 * B or nl in range(B - 1, 2 * B + 2)
    _check_sclass(mp, K, 1, n1, n2, depth, w, "k_pwm2")
    rng = random.Random(n1 * 7 + n2)
    lay = mp.sdot_workspace_layout(K, n1, n2, depth, w)
    ws = mp.alloc_workspace_sdot(K, n1, n2, depth, w, torch_dev)
    ws.fill_(0xFF)
    scratch = ws[lay["scratch"]:lay["scratch"] + 8 * n1].view(torch.int64)
    M, X = 1 << (64 * nl), 1 << (64 * n1)
    last = np.zeros(n2, np.uint64)
    last[n2 - 1] = 1
    kinds = {"random": lambda: np.frombuffer(rng.randbytes(8 * n2), dtype=np.uint64), "ones": lambda: np.full(n2, ONES, np.uint64),
             "zero": lambda: np.zeros(n2, np.uint64), "top limb 1": lambda: last}
    dr = torch.zeros(nl, dtype=torch.int64, device=torch_dev)
    for j in (1, 3, 64):
        for kind, make in kinds.items():
            tot = 0
            for i in range(j):
                b = make()
                a = np.frombuffer(rng.randbytes(8 * n1), dtype=np.uint64)
                tot += to_int(b)
                mp.sdot_stage(mp.STAGE_SD_NEG | (mp.STAGE_ACC if i else 0), K, _t(a, torch_dev), _t(b, torch_dev), None, n1, n2, depth, w, ws)
            torch.cuda.synchronize()
            assert (scratch.cpu().numpy().view(np.uint64) == ~a).all(), (j, kind)
            corr = (X - 1) * tot
            almost = (M - 1 - (1 << (64 * rng.randrange(nl))) + corr) % M   # the result all ones but one limb
            for fill in (rng.getrandbits(64 * nl), 0, M - 1, almost, corr % M):
                dr.copy_(_t(from_int(fill, nl), torch_dev))
                mp.sdot_stage(mp.STAGE_SD_FIX, K, None, None, dr, n1, n2, depth, w, ws)
                torch.cuda.synchronize()
                got = dr.cpu().numpy().view(np.uint64)
                assert (got == from_int((fill - corr) % M, nl)).all(), (j, kind, hex(fill)[:20])


@pytest.mark.parametrize("depth,w,n,kind,head", [(5, 4096, 20000, None, "k_pwss<18>"), (11, 8, 5000, None, "k_pwm2")])
def test_stage_composition(mp, oracle, torch_dev, depth, w, n, kind, head):
    """The driver's stages one by one through sdot_stage: a positive term, then a negative one -- its
    pre-pass, its forward columns on the scratch -- the inverse side once, the correction: equal to
    sdot_device and to the integer value."""
    import torch
    K, neg = 2, 0b10
    with _pointwise_env(kind):
        _check_sclass(mp, K, neg, n, n, depth, w, head)
        pool = _SPool(mp, oracle, torch_dev, n, n, 0x57a + depth)
        names = [("a0", "b0"), ("a1", "b1")]
        lay = mp.sdot_workspace_layout(K, n, n, depth, w)
        ws = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)
        ws.fill_(0x5A)
        scratch = ws[lay["scratch"]:lay["scratch"] + 8 * n].view(torch.int64)
        dr = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
        for i, (a, b) in enumerate(pool.terms(names)):
            if (neg >> i) & 1:
                mp.sdot_stage(mp.STAGE_SD_NEG, K, a, b, None, n, n, depth, w, ws)
                a = scratch
            mp.sdot_stage(mp.STAGE_FWD_COLUMNS, K, a, b, dr, n, n, depth, w, ws)
            mp.sdot_stage(mp.STAGE_FWD_ROWS, K, a, b, dr, n, n, depth, w, ws)
            mp.sdot_stage(mp.STAGE_POINTWISE | (mp.STAGE_ACC if i else 0), K, a, b, dr, n, n, depth, w, ws)
        for st in (mp.STAGE_INV_ROWS, mp.STAGE_INV_COLUMNS, mp.STAGE_SCALE, mp.STAGE_COMBINE, mp.STAGE_SD_FIX):
            mp.sdot_stage(st, K, None, None, dr, n, n, depth, w, ws)
        torch.cuda.synchronize()
        staged = dr.cpu().numpy().view(np.uint64)
        whole = _sdot(mp, torch_dev, pool.terms(names), neg, n, n, depth, w)
    assert (staged == pool.signed(names, neg)[1]).all()
    assert (whole == staged).all()


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (5, 4096, 20000), (11, 8, 5000)])
def test_stays_inside_sdot_workspace_bytes(mp, oracle, torch_dev, depth, w, n):
    """a 0xFF-filled workspace of exactly sdot_workspace_bytes, a guard behind it: D and the chain's
    flags depend on no cleared memory"""
    import torch
    K, neg = 3, 0b110
    nb = mp.sdot_workspace_bytes(K, n, n, depth, w)
    assert nb > 0
    guard = 1 << 20
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf[:nb].fill_(0xFF)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    pool = _SPool(mp, oracle, torch_dev, n, n, 0x99 + w)
    names = [("a0", "b0"), ("a1", "b1"), ("a2", "b2")]
    got = _sdot(mp, torch_dev, pool.terms(names), neg, n, n, depth, w, buf[:nb])
    assert (got == pool.signed(names, neg)[1]).all()
    assert torch.equal(buf[nb:], pat), "the signed sum wrote past mpfft_sdot_workspace_bytes"
    pa = (ctypes.c_void_p * K)(*[a.data_ptr() for a, _ in pool.terms(names)])
    dr = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
    assert mp.lib().mpfft_sdot_device(dr.data_ptr(), K, neg, pa, pa, n, n, depth, w, buf.data_ptr(), nb - 1, None) == ENOMEM
    assert mp.lib().mpfft_sdot_stage(mp.STAGE_SD_FIX, K, None, None, dr.data_ptr(), n, n, depth, w, buf.data_ptr(), nb - 1, None) == ENOMEM


@pytest.mark.parametrize("depth,w,n", [(7, 1024, 131000), (8, 512, 40000), (11, 8, 5000)])
def test_back_to_back_signed_sums_on_one_workspace(mp, oracle, torch_dev, depth, w, n):
    """Two signed sums with different masks queued on one stream with one workspace: the second's first
    negative term initialises D again, and the chain's flags and ticket are cleared again."""
    import torch
    K = 3
    pool = _SPool(mp, oracle, torch_dev, n, n, 0x222 + depth)
    s1 = ([("a0", "b0"), ("1a", "1b"), ("a1", "b1")], 0b011)
    s2 = ([("a1", "b1"), ("a2", "b2"), ("1a", "1b")], 0b100)
    r1, r2 = (torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev) for _ in range(2))
    ws = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for r, (names, neg) in ((r1, s1), (r2, s2)):
            t = pool.terms(names)
            mp.sdot_device(r, [a for a, _ in t], [b for _, b in t], neg, n, n, depth, w, ws, st)
    st.synchronize()
    assert (r1.cpu().numpy().view(np.uint64) == pool.signed(*s1)[1]).all()
    assert (r2.cpu().numpy().view(np.uint64) == pool.signed(*s2)[1]).all()


@pytest.mark.parametrize("K,n1,n2,neg", [(1, 1, 1, [True]), (3, 7, 5, 0b101), (2, 1000, 900, [False, True]), (4, 100000, 100000, 0b0110)])
def test_host_entries(mp, oracle, K, n1, n2, neg):
    a = [mp.fill_random(n1, 0xabc + n1 + i) for i in range(K)]
    b = [mp.fill_random(n2, 0xdef + n2 + i) for i in range(K)]
    mask = mp._neg_mask(neg)
    val = sum((-1 if (mask >> i) & 1 else 1) * to_int(oracle.gmp_mul(x, y)) for i, (x, y) in enumerate(zip(a, b)))
    depth, w = mp.dot_choose(K, n1, n2)
    got = mp.sdot(a, b, neg, depth, w)
    assert (got == _twos(val, n1 + n2 + 1)).all(), (K, n1, n2, depth, w)
    assert mp.sdot_to_int(got) == val
    assert (mp.sdot_auto(a, b, neg) == got).all(), (K, n1, n2)


def test_profile_covers_signed_sums(mp, oracle, torch_dev):
    """seven finite stage times, a call slot per term, with the pre-pass and the correction inside"""
    depth, w, n, K, neg = 8, 512, 40000, 3, 0b101
    pool = _SPool(mp, oracle, torch_dev, n, n, 0x321)
    names = [("a0", "b0"), ("a1", "b1"), ("a2", "b2")]
    ws = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)
    mp.profile_begin(K)
    got = _sdot(mp, torch_dev, pool.terms(names), neg, n, n, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == K
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert ms["pointwise"] > 0 and ms["fwd_columns"] > 0 and ms["combine"] > 0, ms
    assert (got == pool.signed(names, neg)[1]).all()


def test_c_caller_sdot(mp):
    exe = os.path.join(HERE, "c_sdot", "sdot_caller")
    assert os.path.exists(exe), "tests/c_sdot/sdot_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
