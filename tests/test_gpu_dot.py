"""GPU tests of the sums of products (mpfft_dot_*): r = sum_i a_i b_i with one inverse transform.

Whole sums through every pointwise class (k_pwss + k_pwsa<10/18/20> at FUSE 0, pair and quad;
k_pwm2, k_pwm, k_pw, k_pointwise + k_slotacc), the coefficient bound at its tightest, unbalanced
operands, K = 1 against the multiply, a non-zero top limb, the stages composed by hand, the
accumulating pointwise alone on placed residues and on hand-placed reduced-form accumulators, the
workspace size, back-to-back calls, the host entries, profiling and a plain C caller.  The reference
is Python integers, or GMP products (oracle.gmp_mul) added as integers; bit-exact is the only bar.
Every case asserts its kernel class through dot_stage_kernels first."""
import ctypes
import math
import os
import random
import subprocess

import numpy as np
import pytest

import stage_model
from helpers import from_int, to_int
from test_gpu_sqr import PAIR, WHOLE, _modp, _pattern, _pointwise_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def _check_class(mp, K, n1, n2, depth, w, head, has=None, scale=None, combine=None):
    """head: the multiply's pointwise kernel of the class (k_pwss<M>, k_pwm2, ...); has: the pair / quad
    suffix, () for FUSE 0, None for whichever the plan takes"""
    sk = mp.dot_stage_kernels(K, n1, n2, depth, w)
    pw = sk["pointwise"]
    first, later = pw.split(" + k_")
    later = "k_" + later
    assert first.startswith(head), (K, depth, w, n1, n2, pw)
    if head.startswith("k_pwss"):
        assert later == first.replace("k_pwss", "k_pwsa"), pw
        for s in has or ():
            assert s in first, pw
        if has == ():
            assert "pair" not in pw and "quad" not in pw, pw   # FUSE 0
    else:
        assert later == "k_slotacc", pw
    if scale:
        assert sk["scale"].startswith(scale), sk["scale"]
    if combine:
        assert sk["combine"].startswith(combine), sk["combine"]
    return sk


def _dot(mp, dev, terms, n1, n2, depth, w, ws=None):
    """terms: (a tensor, b tensor) per term; the n1 + n2 + 1 limbs of the sum"""
    import torch
    K = len(terms)
    dr = torch.full((n1 + n2 + 1,), 0x5a5a5a5a, dtype=torch.int64, device=dev)
    if ws is None:
        ws = mp.alloc_workspace_dot(K, n1, n2, depth, w, dev)
    mp.dot_device(dr, [a for a, _ in terms], [b for _, b in terms], n1, n2, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _ones_product(n1, n2):
    """(2^(64 n1) - 1) (2^(64 n2) - 1), without a multiplication of that size"""
    return (1 << (64 * (n1 + n2))) - (1 << (64 * n1)) - (1 << (64 * n2)) + 1


class _Pool:
    """named operands on the device and their GMP products, each computed once"""

    def __init__(self, mp, oracle, dev, n1, n2, seed):
        self.oracle, self.n1, self.n2 = oracle, n1, n2
        self.h = {"a0": mp.fill_random(n1, seed), "a1": mp.fill_random(n1, seed + 1), "a2": mp.fill_random(n1, seed + 2),
                  "b0": mp.fill_random(n2, seed + 3), "b1": mp.fill_random(n2, seed + 4), "b2": mp.fill_random(n2, seed + 5),
                  "1a": np.full(n1, 2**64 - 1, np.uint64), "1b": np.full(n2, 2**64 - 1, np.uint64),
                  "0a": np.zeros(n1, np.uint64)}
        self.d = {k: _t(v, dev) for k, v in self.h.items()}
        self.prod = {}

    def want(self, names):
        tot = 0
        for x, y in names:
            key = (x, y)
            if key not in self.prod:
                if x == "0a":
                    self.prod[key] = 0
                elif x[0] == "1" and y[0] == "1":
                    self.prod[key] = _ones_product(self.n1, self.n2)
                else:
                    self.prod[key] = to_int(self.oracle.gmp_mul(self.h[x], self.h[y]))
            tot += self.prod[key]
        return from_int(tot, self.n1 + self.n2 + 1)

    def terms(self, names):
        return [(self.d[x], self.d[y]) for x, y in names]


def _operand_sets(K):
    """(label, term names): random operands, every term all-ones, one term with a zero operand,
    a_0 == b_0 aliased (n1 == n2), the same pointer in two terms"""
    rnd = [("a0", "b0"), ("a1", "b1"), ("a2", "b2"), ("a1", "b0")][:K]
    return [("random", rnd),
            ("all-ones", [("1a", "1b")] * K),
            ("zero operand", rnd[:-1] + [("0a", rnd[-1][1])]),
            ("a_0 == b_0", [("a0", "a0")] + rnd[1:]),
            ("repeated pointer", [("a0", "b0")] + [("a0", y) for _, y in rnd[1:]])]


def _whole(mp, oracle, dev, K, depth, w, n, kind, head, has, scale, combine, caseb):
    head = head.replace("k_pwsq", "k_pwss")
    if n is None:
        n = mp.dot_max_limbs(K, depth, w)
    with _pointwise_env(kind):
        assert mp.dot_check_params(K, n, n, depth, w) == 0, (K, depth, w, n)
        sk = _check_class(mp, K, n, n, depth, w, head, has, scale, combine)
        if caseb:
            P = mp.dot_plan_info(K, n, n, depth, w)
            assert P["trunc"] > P["n"]
        ws = mp.alloc_workspace_dot(K, n, n, depth, w, dev)
        pool = _Pool(mp, oracle, dev, n, n, 0xd07 + 31 * depth + w)
        for label, names in _operand_sets(K):
            got = _dot(mp, dev, pool.terms(names), n, n, depth, w, ws)
            assert (got == pool.want(names)).all(), (label, K, depth, w, n, sk["pointwise"])


@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine,caseb", WHOLE)
def test_whole_sums_of_two_every_pointwise_class(mp, oracle, torch_dev, depth, w, n, kind, head, has, scale, combine, caseb):
    _whole(mp, oracle, torch_dev, 2, depth, w, n, kind, head, has, scale, combine, caseb)


# one FUSE 0, one pair and one quad shape of WHOLE
MORE = [s for s in WHOLE if s[:3] in ((5, 4096, 20000), (8, 512, 140000), (14, 8, 500000))]


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine,caseb", MORE)
def test_whole_sums_of_three_and_four(mp, oracle, torch_dev, K, depth, w, n, kind, head, has, scale, combine, caseb):
    assert len(MORE) == 3
    _whole(mp, oracle, torch_dev, K, depth, w, n, kind, head, has, scale, combine, caseb)


# (depth, w, MPFFT_POINTWISE, class): the small k_pointwise / k_pw shapes and the nested ones
TIGHT = [(9, 2, None, "k_pointwise"), (8, 8, None, "k_pw "), (10, 2, None, "k_pw "), (9, 16, None, "k_pwm "), (8, 64, None, "k_pwm2"),
         (5, 4096, None, "k_pwss<18>"), (6, 4096, None, "k_pwss<20>"), (6, 1024, "pwss", "k_pwss<10>")]


@pytest.mark.parametrize("K", [2, 3, 64])
def test_the_bound_tight(mp, torch_dev, K):
    """All-ones operands at n1 = n2 = dot_max_limbs: the largest coefficients the plan admits (below
    2^N by K 2^depth (2^bits1 - 1)^2 < 2^(s + depth + 2 bits1) alone).  An implementation that kept
    the multiply's bits1 fails the shapes where N - depth - s is even."""
    s = (K - 1).bit_length()
    even = 0
    for depth, w, kind, head in TIGHT:
        N = (1 << depth) * w
        even += (N - depth - s) % 2 == 0
        n = mp.dot_max_limbs(K, depth, w)
        with _pointwise_env(kind):
            P = mp.dot_plan_info(K, n, n, depth, w)
            assert P["bits1"] == (N - depth - s) // 2 and P["j1"] == 1 << depth
            _check_class(mp, K, n, n, depth, w, head)
            ones = _t(np.full(n, 2**64 - 1, np.uint64), torch_dev)
            got = _dot(mp, torch_dev, [(ones, ones)] * K, n, n, depth, w)
        assert to_int(got) == K * _ones_product(n, n), (K, depth, w, n)
    assert even >= 1


@pytest.mark.parametrize("depth,w,n1,n2,head,has", [(8, 512, 220000, 60000, "k_pwss<18>", (PAIR,)), (8, 512, 60000, 220000, "k_pwss<18>", (PAIR,)),
                                                    (11, 8, 300000, 30000, "k_pwm2", ()), (11, 8, 30000, 300000, "k_pwm2", ())])
def test_unbalanced_in_truncation_case_b(mp, oracle, torch_dev, depth, w, n1, n2, head, has):
    K = 3
    P = mp.dot_plan_info(K, n1, n2, depth, w)
    assert P["trunc"] > P["n"] and P["trunc"] < 2 * P["n"]
    _check_class(mp, K, n1, n2, depth, w, head, has)
    pool = _Pool(mp, oracle, torch_dev, n1, n2, 0xb1 + depth)
    names = [("a0", "b0"), ("a1", "b1"), ("1a", "1b")]
    got = _dot(mp, torch_dev, pool.terms(names), n1, n2, depth, w)
    assert (got == pool.want(names)).all()


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (5, 4096, 20000), (11, 8, 5000), (9, 2, 120)])
def test_one_term_is_the_multiply(mp, torch_dev, depth, w, n):
    import torch
    assert mp.dot_plan_info(1, n, n, depth, w) == mp.plan_info(n, n, depth, w)
    a, b = _t(mp.fill_random(n, 0x1a), torch_dev), _t(mp.fill_random(n, 0x1b), torch_dev)
    dm = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    mp.mul_device(dm, a, n, b, n, depth, w, mp.alloc_workspace(n, n, depth, w, torch_dev))
    got = _dot(mp, torch_dev, [(a, b)], n, n, depth, w)
    assert (got[:2 * n] == dm.cpu().numpy().view(np.uint64)).all()
    assert got[2 * n] == 0


def test_a_sum_with_a_top_limb(mp, torch_dev):
    depth, w, n, K = 9, 2, 120, 64
    _check_class(mp, K, n, n, depth, w, "k_pointwise")
    ones = _t(np.full(n, 2**64 - 1, np.uint64), torch_dev)
    got = _dot(mp, torch_dev, [(ones, ones)] * K, n, n, depth, w)
    assert to_int(got) == K * _ones_product(n, n)
    assert got[2 * n] == K - 1


@pytest.mark.parametrize("depth,w,n,kind,head", [(5, 4096, 20000, None, "k_pwss<18>"), (6, 1024, 30000, "pwss", "k_pwss<10>"),
                                                 (6, 4096, 100000, None, "k_pwss<20>"), (11, 8, 5000, None, "k_pwm2"),
                                                 (9, 2, 120, None, "k_pointwise")])
def test_stage_composition(mp, oracle, torch_dev, depth, w, n, kind, head):
    """The driver's stages one by one through dot_stage: two terms' forward stages and pointwise (the
    second accumulating), then the inverse side once -- equal to dot_device and to the integer sum."""
    import torch
    K = 2
    with _pointwise_env(kind):
        _check_class(mp, K, n, n, depth, w, head)
        pool = _Pool(mp, oracle, torch_dev, n, n, 0x57a + depth)
        names = [("a0", "b0"), ("a1", "b1")]
        ws = mp.alloc_workspace_dot(K, n, n, depth, w, torch_dev)
        ws.fill_(0x5A)
        dr = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
        for i, (a, b) in enumerate(pool.terms(names)):
            mp.dot_stage(mp.STAGE_FWD_COLUMNS, K, a, b, dr, n, n, depth, w, ws)
            mp.dot_stage(mp.STAGE_FWD_ROWS, K, a, b, dr, n, n, depth, w, ws)
            mp.dot_stage(mp.STAGE_POINTWISE | (mp.STAGE_ACC if i else 0), K, a, b, dr, n, n, depth, w, ws)
        for st in (mp.STAGE_INV_ROWS, mp.STAGE_INV_COLUMNS, mp.STAGE_SCALE, mp.STAGE_COMBINE):
            mp.dot_stage(st, K, None, None, dr, n, n, depth, w, ws)
        torch.cuda.synchronize()
        staged = dr.cpu().numpy().view(np.uint64)
        whole = _dot(mp, torch_dev, pool.terms(names), n, n, depth, w)
    assert (staged == pool.want(names)).all()
    assert (whole == staged).all()


# ---- the accumulating pointwise alone ------------------------------------------------------------
# per nested M and one shape of each other family
PLACED = [(5, 4096, None, "k_pwss<18>"), (6, 4096, None, "k_pwss<20>"), (6, 1024, "pwss", "k_pwss<10>"),
          (9, 16, None, "k_pwm "), (8, 64, None, "k_pwm2"), (11, 1, None, "k_pw "), (9, 2, None, "k_pointwise")]


def _place(views, x, T, vals, dev):
    """canonical residues (v, top) into slots [0, T) of array x, carry masks zero"""
    import torch
    dig, top, cb = views[x]
    l = dig.shape[1]
    hd = np.zeros((T, l), np.uint64)
    for s, (v, _) in enumerate(vals):
        hd[s] = np.frombuffer(v.to_bytes(8 * l, "little"), dtype=np.uint64)
    dig[:T] = torch.from_numpy(hd.view(np.int64)).to(dev)
    top[:T] = torch.from_numpy(np.array([t for _, t in vals], np.int32)).to(dev)
    cb[:T] = 0


def _read_c(views, T, N):
    """slots [0, T) of C as integers: limbs + carries + top 2^N (stage_model.unpack_value)"""
    dig, top, cb = (x.cpu().numpy() for x in views["C"])
    dig, cb = dig.view(np.uint64), cb.view(np.uint64)
    return [stage_model.unpack_value(dig[s], int(top[s]), cb[s], N) for s in range(T)]


def _setup_placed(mp, dev, depth, w, head):
    K = 2
    n = mp.dot_max_limbs(K, depth, w)
    P = mp.dot_plan_info(K, n, n, depth, w)
    _check_class(mp, K, n, n, depth, w, head)
    ws = mp.alloc_workspace_dot(K, n, n, depth, w, dev)
    ws.fill_(0)
    return K, n, P["l"], P["trunc"], P["n"] * w, ws, mp.dot_workspace_views(ws, K, n, n, depth, w)


@pytest.mark.parametrize("depth,w,kind,head", PLACED)
def test_accumulating_pointwise_on_placed_residues(mp, torch_dev, depth, w, kind, head):
    """C <- A0 B0 by POINTWISE, then C <- C + A1 B1 by POINTWISE | ACC, every ordered pair of the eight
    patterns as (A1, B1): each live slot of C against (A0 B0 + A1 B1) mod 2^N + 1."""
    import torch
    rng = random.Random(depth * 1000 + w)
    with _pointwise_env(kind):
        K, n, l, T, N, ws, views = _setup_placed(mp, torch_dev, depth, w, head)
        assert T >= 64
        p = (1 << N) + 1
        pats = [_pattern(k, l, N, rng) for k in range(8)]
        A0 = [pats[(s // 8 + s) % 8] for s in range(T)]
        B0 = [pats[(s + 5) % 8] for s in range(T)]
        A1 = [pats[s % 8] if s < 64 else _pattern(0, l, N, rng) for s in range(T)]
        B1 = [pats[(s // 8) % 8] for s in range(T)]
        assert len({(A1[s], B1[s]) for s in range(64)}) == 64
        z = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
        _place(views, "A", T, A0, torch_dev)
        _place(views, "B", T, B0, torch_dev)
        mp.dot_stage(mp.STAGE_POINTWISE, K, z, z, z, n, n, depth, w, ws)
        torch.cuda.synchronize()
        val = lambda x: x[0] + x[1] * (1 << N)
        first = [_modp(val(A0[s]) * val(B0[s]), N) for s in range(T)]
        bad = [s for s, v in enumerate(_read_c(views, T, N)) if v % p != first[s]]
        assert not bad, f"C <- A B: {len(bad)} of {T} slots wrong, first {bad[:8]}"
        _place(views, "A", T, A1, torch_dev)
        _place(views, "B", T, B1, torch_dev)
        mp.dot_stage(mp.STAGE_POINTWISE | mp.STAGE_ACC, K, z, z, z, n, n, depth, w, ws)
        torch.cuda.synchronize()
        bad = [s for s, v in enumerate(_read_c(views, T, N)) if v % p != (first[s] + _modp(val(A1[s]) * val(B1[s]), N)) % p]
    assert not bad, f"C <- C + A B: {len(bad)} of {T} slots wrong, first {bad[:8]}"


def _accumulators(l, rng):
    """hand-placed reduced-form encodings (limbs, +1 carries, -1 carries, top)"""
    rnd = lambda: np.frombuffer(rng.randbytes(8 * l), dtype=np.uint64).copy()
    ones, zero = np.full(l, 2**64 - 1, np.uint64), np.zeros(l, np.uint64)
    out = []
    for top in (-1, 0, 1):   # random limbs, random disjoint +1 / -1 mask bits on every limb
        c = [rng.choice((0, 1, -1)) for _ in range(l)]
        out.append((rnd(), {m for m in range(l) if c[m] == 1}, {m for m in range(l) if c[m] == -1}, top))
    out.append((rnd(), {l - 1}, set(), 0))            # a carry of each sign out of limb l - 1
    out.append((rnd(), set(), {l - 1}, 0))
    out.append((rnd(), {l - 1}, set(), 1))            # ... together with the top
    out.append((rnd(), set(), {l - 1}, -1))
    out.append((rnd(), set(), set(), 1))              # top alone
    out.append((rnd(), set(), set(), -1))
    for limbs in (ones, zero):                        # all-ones and all-zero limb rows: the carries ripple
        out.append((limbs.copy(), set(), set(), 0))
        out.append((limbs.copy(), set(range(l)), set(), 1))
        out.append((limbs.copy(), set(), set(range(l)), -1))
        out.append((limbs.copy(), set(range(0, l, 2)), set(range(1, l, 2)), 0))
        out.append((limbs.copy(), {0, l - 1}, {l // 2}, -1))
    return out


@pytest.mark.parametrize("depth,w,kind,head", PLACED)
def test_accumulating_pointwise_on_placed_accumulators(mp, torch_dev, depth, w, kind, head):
    """C hand-placed in the reduced form -- pending +-1 carries on every limb, the carry out of limb
    l - 1, top in {-1, 1}, all-ones and all-zero limbs -- times a product of 2^N 2^N, of 0 and a
    random one: POINTWISE | ACC against (C + A B) mod 2^N + 1.  An accumulator that dropped the old
    carries or the top fails here."""
    import torch
    rng = random.Random(depth * 77 + w)
    with _pointwise_env(kind):
        K, n, l, T, N, ws, views = _setup_placed(mp, torch_dev, depth, w, head)
        p = (1 << N) + 1
        accs = _accumulators(l, rng)
        prods = [((0, 1), (0, 1)), ((0, 0), _pattern(0, l, N, rng)), None]   # 2^N 2^N; 0; random
        assert T >= len(accs) * len(prods)
        cbw = views["C"][2].shape[1]
        digC, topC, cbC = views["C"]
        hd, ht, hc = np.zeros((T, l), np.uint64), np.zeros(T, np.int32), np.zeros((T, cbw), np.uint64)
        A, B, want = [], [], []
        enc = []   # per encoding: limbs, top, mask words, value
        for limbs, pos, neg, top in accs:
            words = stage_model.pack_masks(pos, neg, cbw)
            enc.append((limbs, top, words, stage_model.val_reduced(limbs, pos, neg, top, N)))
            assert enc[-1][3] == stage_model.unpack_value(limbs, top, words, N)
        for s in range(T):
            hd[s], ht[s], hc[s], old = enc[s % len(accs)]
            pr = prods[(s // len(accs)) % len(prods)] or (_pattern(0, l, N, rng), _pattern(7, l, N, rng))
            A.append(pr[0])
            B.append(pr[1])
            want.append((old + (pr[0][0] + pr[0][1] * (1 << N)) * (pr[1][0] + pr[1][1] * (1 << N))) % p)
        digC[:T] = torch.from_numpy(hd.view(np.int64)).to(torch_dev)
        topC[:T] = torch.from_numpy(ht).to(torch_dev)
        cbC[:T] = torch.from_numpy(hc.view(np.int64)).to(torch_dev)
        _place(views, "A", T, A, torch_dev)
        _place(views, "B", T, B, torch_dev)
        z = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
        mp.dot_stage(mp.STAGE_POINTWISE | mp.STAGE_ACC, K, z, z, z, n, n, depth, w, ws)
        torch.cuda.synchronize()
        bad = [s for s, v in enumerate(_read_c(views, T, N)) if v % p != want[s]]
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]} (encoding {[b % len(accs) for b in bad[:8]]})"


# ---- the rest ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (5, 4096, 20000), (11, 8, 5000)])
def test_stays_inside_dot_workspace_bytes(mp, oracle, torch_dev, depth, w, n):
    import torch
    K = 3
    nb = mp.dot_workspace_bytes(K, n, n, depth, w)
    assert nb > 0
    guard = 1 << 20
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf[:nb].fill_(0xFF)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    pool = _Pool(mp, oracle, torch_dev, n, n, 0x99 + w)
    names = [("a0", "b0"), ("a1", "b1"), ("a2", "b2")]
    got = _dot(mp, torch_dev, pool.terms(names), n, n, depth, w, buf[:nb])
    assert (got == pool.want(names)).all()
    assert torch.equal(buf[nb:], pat), "the sum wrote past mpfft_dot_workspace_bytes"
    ENOMEM = 4
    pa = (ctypes.c_void_p * K)(*[a.data_ptr() for a, _ in pool.terms(names)])
    dr = torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev)
    assert mp.lib().mpfft_dot_device(dr.data_ptr(), K, pa, pa, n, n, depth, w, buf.data_ptr(), nb - 1, None) == ENOMEM


@pytest.mark.parametrize("depth,w,n", [(7, 1024, 131000), (8, 512, 40000), (11, 8, 5000)])
def test_back_to_back_sums_on_one_workspace(mp, oracle, torch_dev, depth, w, n):
    """Two sums queued on one stream with one workspace: the second's first term overwrites the
    accumulator, and its first pass clears the combine's look-back flags again."""
    import torch
    K = 2
    pool = _Pool(mp, oracle, torch_dev, n, n, 0x222 + depth)
    n1 = [("a0", "b0"), ("1a", "1b")]
    n2 = [("a1", "b1"), ("a2", "b2")]
    r1, r2 = (torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev) for _ in range(2))
    ws = mp.alloc_workspace_dot(K, n, n, depth, w, torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for r, names in ((r1, n1), (r2, n2)):
            t = pool.terms(names)
            mp.dot_device(r, [a for a, _ in t], [b for _, b in t], n, n, depth, w, ws, st)
    st.synchronize()
    assert (r1.cpu().numpy().view(np.uint64) == pool.want(n1)).all()
    assert (r2.cpu().numpy().view(np.uint64) == pool.want(n2)).all()


@pytest.mark.parametrize("K,n1,n2", [(1, 1, 1), (3, 7, 5), (2, 1000, 900), (4, 100000, 100000), (2, 1500000, 1500000)])
def test_host_entries(mp, oracle, K, n1, n2):
    a = [mp.fill_random(n1, 0xabc + n1 + i) for i in range(K)]
    b = [mp.fill_random(n2, 0xdef + n2 + i) for i in range(K)]
    want = from_int(sum(to_int(oracle.gmp_mul(x, y)) for x, y in zip(a, b)), n1 + n2 + 1)
    depth, w = mp.dot_choose(K, n1, n2)
    assert (mp.dot(a, b, depth, w) == want).all(), (K, n1, n2, depth, w)
    assert (mp.dot_auto(a, b) == want).all(), (K, n1, n2)


def test_profile_covers_sums(mp, oracle, torch_dev):
    """seven stage times; every term claims a call slot, the forward and pointwise times add up"""
    depth, w, n, K = 8, 512, 40000, 3
    pool = _Pool(mp, oracle, torch_dev, n, n, 0x321)
    names = [("a0", "b0"), ("a1", "b1"), ("a2", "b2")]
    ws = mp.alloc_workspace_dot(K, n, n, depth, w, torch_dev)
    mp.profile_begin(K)
    got = _dot(mp, torch_dev, pool.terms(names), n, n, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == K
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert ms["pointwise"] > 0 and ms["fwd_columns"] > 0 and ms["inv_rows"] > 0, ms
    assert (got == pool.want(names)).all()


def test_c_caller_dot(mp):
    exe = os.path.join(HERE, "c_dot", "dot_caller")
    assert os.path.exists(exe), "tests/c_dot/dot_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
