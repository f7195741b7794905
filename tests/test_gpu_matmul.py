"""GPU tests of the small matrix products (mpfft_matmul_*): R = X Y with every operand forward-transformed
once and one inverse transform per result entry.

Whole 2x2 by 2x2 products through every pointwise class (k_pwsx + k_pwmm<10/18/20> at FUSE 0, pair and quad;
k_pwm2, k_pwm, k_pw, k_pointwise with cached B + k_slotacc), back to back on one workspace where the combine
reads the reduced form, the other shapes, the coefficient bound and the inner accumulator at their tightest,
(1, 1, 1) against the multiply, zero and repeated operands, unbalanced entries, k_pwmm alone on placed
residues and on hand-placed reduced-form accumulators, the workspace size, limb-aligned and scattered
pointers, two streams, the host entries, profiling and a plain C caller.  The reference is GMP products
(oracle.gmp_mul) summed as Python integers, and mpfft_dot_device limb for limb; bit-exact is the only bar.
Every case asserts its kernel class through matmul_stage_kernels first."""
import ctypes
import math
import os
import random
import subprocess

import numpy as np
import pytest

import stage_model
from helpers import from_int, to_int
from test_gpu_sqr import WHOLE, _modp, _pattern, _pointwise_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FOLD = "k_cmeta + k_combine_red"


def _mm():
    """the bindings of this family: the submodule mpir_fft_amd.matmul (the package is loaded by the mp fixture)"""
    import mpir_fft_amd.matmul
    return mpir_fft_amd.matmul


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def _ones_product(n1, n2):
    """(2^(64 n1) - 1) (2^(64 n2) - 1), without a multiplication of that size"""
    return (1 << (64 * (n1 + n2))) - (1 << (64 * n1)) - (1 << (64 * n2)) + 1


def _check_class(mp, m, k, p, n1, n2, depth, w, head, has=None, scale=None, combine=None):
    """head: the multiply's pointwise kernel of the class (k_pwss<M>, k_pwm2, ...); has: the pair / quad
    suffix, () for FUSE 0, None for whichever the plan takes"""
    sk = _mm().matmul_stage_kernels(m, k, p, n1, n2, depth, w)
    pw = sk["pointwise"]
    first, later = pw.split(" + k_")
    later = "k_" + later
    if head.startswith("k_pwss"):
        M = head[len("k_pwss"):]
        assert first.startswith("k_pwsx" + M), (m, k, p, depth, w, n1, n2, pw)
        assert later.startswith("k_pwmm" + M), pw
        for s in has or ():
            assert s in first, pw
        if has == ():
            assert "pair" not in pw and "quad" not in pw, pw   # FUSE 0
    else:
        assert first.startswith(head) and first.endswith("(B cached)"), (m, k, p, depth, w, n1, n2, pw)
        assert later == "k_slotacc", pw
    if scale:
        assert sk["scale"].startswith(scale), sk["scale"]
    if combine:
        assert sk["combine"].startswith(combine), sk["combine"]
    return sk


class _Ops:
    """named operands on the device ("x..." of n1 limbs, "y..." of n2) and their GMP products, each computed once"""

    def __init__(self, mp, oracle, dev, n1, n2, seed):
        self.mp, self.oracle, self.dev, self.n1, self.n2, self.seed = mp, oracle, dev, n1, n2, seed
        self.h, self.d, self.prod = {}, {}, {}

    def host(self, name):
        if name not in self.h:
            n = self.n1 if name[0] == "x" else self.n2
            if name[1:] == "ones":
                self.h[name] = np.full(n, 2**64 - 1, np.uint64)
            elif name[1:] == "zero":
                self.h[name] = np.zeros(n, np.uint64)
            else:
                self.h[name] = self.mp.fill_random(n, self.seed + 2 * int(name[1:]) + (name[0] == "y"))
            self.d[name] = _t(self.h[name], self.dev)
        return self.h[name]

    def dev_of(self, name):
        self.host(name)
        return self.d[name]

    def product(self, x, y):
        if (x, y) not in self.prod:
            a, b = self.host(x), self.host(y)
            if "zero" in (x[1:], y[1:]):
                v = 0
            elif x[1:] == "ones" and y[1:] == "ones":
                v = _ones_product(len(a), len(b))
            else:
                v = to_int(self.oracle.gmp_mul(a, b))
            self.prod[(x, y)] = v
        return self.prod[(x, y)]

    def want(self, X, Y, m, k, p):
        """the m p result entries (limb arrays), row-major, from the names in X (m k) and Y (k p)"""
        return [from_int(sum(self.product(X[i * k + t], Y[t * p + j]) for t in range(k)), self.n1 + self.n2 + 1)
                for i in range(m) for j in range(p)]


def _names(m, k, p, base=0):
    """distinct random entries: a transposed or swapped index fails"""
    return ["x%d" % (base + e) for e in range(m * k)], ["y%d" % (base + e) for e in range(k * p)]


def _matmul(mp, ops, X, Y, m, k, p, depth, w, ws=None, stream=None, rs=None):
    import torch
    n1, n2 = ops.n1, ops.n2
    if rs is None:
        rs = [torch.full((n1 + n2 + 1,), 0x5a5a5a5a, dtype=torch.int64, device=ops.dev) for _ in range(m * p)]
    if ws is None:
        ws = _mm().alloc_workspace_matmul(m, k, p, n1, n2, depth, w, ops.dev)
    _mm().matmul_device(rs, m, k, p, [ops.dev_of(x) for x in X], [ops.dev_of(y) for y in Y], n1, n2, depth, w, ws, stream)
    return rs


def _limbs(rs):
    import torch
    torch.cuda.synchronize()
    return [r.cpu().numpy().view(np.uint64) for r in rs]


def _dots(mp, ops, X, Y, m, k, p, depth, w):
    """every result entry through mpfft_dot_device on its k terms"""
    import torch
    wd = mp.alloc_workspace_dot(k, ops.n1, ops.n2, depth, w, ops.dev)
    out = []
    for i in range(m):
        for j in range(p):
            d = torch.zeros(ops.n1 + ops.n2 + 1, dtype=torch.int64, device=ops.dev)
            mp.dot_device(d, [ops.dev_of(X[i * k + t]) for t in range(k)], [ops.dev_of(Y[t * p + j]) for t in range(k)],
                          ops.n1, ops.n2, depth, w, wd)
            torch.cuda.synchronize()
            out.append(d.cpu().numpy().view(np.uint64))
    return out


def _assert_entries(got, want, what):
    assert len(got) == len(want)
    for e, (g, v) in enumerate(zip(got, want)):
        assert (g == v).all(), (what, "entry", e, "limbs differing", int((g != v).sum()))


# ---- whole products ---------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine,caseb", WHOLE)
def test_whole_2x2_every_pointwise_class(mp, oracle, torch_dev, depth, w, n, kind, head, has, scale, combine, caseb):
    """2x2 by 2x2 with eight distinct random entries: every entry against the integer sum and limb for limb
    against dot_device.  Where the combine reads the reduced form (its look-back flags and ticket counter
    are cleared by the forward side in a multiply), two products back to back on one workspace: a stale
    flag or ticket shows from the second result entry on."""
    m = k = p = 2
    head = head.replace("k_pwsq", "k_pwss")
    with _pointwise_env(kind):
        if n is None or mp.dot_check_params(k, n, n, depth, w) != 0:
            n = mp.dot_max_limbs(k, depth, w)
        assert _mm().matmul_check_params(m, k, p, n, n, depth, w) == 0, (depth, w, n)
        sk = _check_class(mp, m, k, p, n, n, depth, w, head, has, scale, combine)
        if caseb:
            P = mp.dot_plan_info(k, n, n, depth, w)
            assert P["trunc"] > P["n"]
        ops = _Ops(mp, oracle, torch_dev, n, n, 0x3a7 + 31 * depth + w)
        ws = _mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev)
        X, Y = _names(m, k, p)
        runs = [(X, Y, _matmul(mp, ops, X, Y, m, k, p, depth, w, ws))]
        if combine == FOLD:
            X2, Y2 = _names(m, k, p, 8)
            runs.append((X2, Y2, _matmul(mp, ops, X2, Y2, m, k, p, depth, w, ws)))
        for Xn, Yn, rs in runs:
            got = _limbs(rs)
            _assert_entries(got, ops.want(Xn, Yn, m, k, p), (depth, w, n, sk["pointwise"]))
            _assert_entries(got, _dots(mp, ops, Xn, Yn, m, k, p, depth, w), "dot_device")
    assert len(runs) == (2 if (depth, w) in ((5, 4096), (6, 2048), (7, 2048)) else 1)


# a nested (pair) and a k_pwm2 shape, n1 != n2 so that a row / column mix-up changes sizes too
SHAPE_PLANS = [(8, 512, 40000, 30000, None, "k_pwss<18>"), (11, 8, 5000, 4000, None, "k_pwm2")]


@pytest.mark.parametrize("m,k,p", [(2, 2, 1), (1, 2, 2), (2, 3, 4), (4, 1, 2), (3, 3, 3)])
@pytest.mark.parametrize("depth,w,n1,n2,kind,head", SHAPE_PLANS)
def test_shapes(mp, oracle, torch_dev, m, k, p, depth, w, n1, n2, kind, head):
    with _pointwise_env(kind):
        _check_class(mp, m, k, p, n1, n2, depth, w, head)
        ops = _Ops(mp, oracle, torch_dev, n1, n2, 0x5a9 + depth + 7 * m + 3 * p)
        X, Y = _names(m, k, p)
        got = _limbs(_matmul(mp, ops, X, Y, m, k, p, depth, w))
    _assert_entries(got, ops.want(X, Y, m, k, p), (m, k, p, depth, w))


@pytest.mark.parametrize("depth,w,kind,head", [(6, 1024, "pwss", "k_pwss<10>"), (5, 4096, None, "k_pwss<18>"),
                                               (6, 4096, None, "k_pwss<20>")])
def test_4x4_all_ones_at_the_bound(mp, torch_dev, depth, w, kind, head):
    """Every entry all-ones at n = dot_max_limbs(4): the outer coefficient bound at its tightest and the
    inner accumulator's top at its largest; one tensor at all 32 places."""
    import torch
    m = k = p = 4
    with _pointwise_env(kind):
        n = mp.dot_max_limbs(k, depth, w)
        assert _mm().matmul_check_params(m, k, p, n, n, depth, w) == 0 and _mm().matmul_check_params(m, k, p, n + 1, n + 1, depth, w) != 0
        _check_class(mp, m, k, p, n, n, depth, w, head)
        ones = _t(np.full(n, 2**64 - 1, np.uint64), torch_dev)
        rs = [torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev) for _ in range(m * p)]
        ws = _mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev)
        _mm().matmul_device(rs, m, k, p, [ones] * (m * k), [ones] * (k * p), n, n, depth, w, ws)
        got = _limbs(rs)
    want = from_int(k * _ones_product(n, n), 2 * n + 1)
    _assert_entries(got, [want] * (m * p), (depth, w, n))
    assert int(got[0][2 * n]) == k - 1


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (5, 4096, 20000), (11, 8, 5000), (9, 2, 120)])
def test_1x1x1_is_the_multiply(mp, torch_dev, depth, w, n):
    import torch
    a, b = _t(mp.fill_random(n, 0x1a), torch_dev), _t(mp.fill_random(n, 0x1b), torch_dev)
    dm = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    mp.mul_device(dm, a, n, b, n, depth, w, mp.alloc_workspace(n, n, depth, w, torch_dev))
    r = torch.full((2 * n + 1,), -1, dtype=torch.int64, device=torch_dev)
    _mm().matmul_device([r], 1, 1, 1, [a], [b], n, n, depth, w, _mm().alloc_workspace_matmul(1, 1, 1, n, n, depth, w, torch_dev))
    got = _limbs([r])[0]
    assert (got[:2 * n] == dm.cpu().numpy().view(np.uint64)).all()
    assert got[2 * n] == 0


@pytest.mark.parametrize("depth,w,n,kind,head", [(8, 512, 40000, None, "k_pwss<18>"), (11, 8, 5000, None, "k_pwm2")])
def test_operand_sets(mp, oracle, torch_dev, depth, w, n, kind, head):
    """a zero entry, a zero row, every pointer the same operand, X[0][0] == Y[0][0] (n1 == n2)"""
    m = k = p = 2
    with _pointwise_env(kind):
        _check_class(mp, m, k, p, n, n, depth, w, head)
        ops = _Ops(mp, oracle, torch_dev, n, n, 0x0b5 + depth)
        ws = _mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev)
        X, Y = _names(m, k, p)
        sets = [("zero entry", [X[0], "xzero", X[2], X[3]], Y),
                ("zero row", ["xzero", "xzero", X[2], X[3]], Y),
                ("zero column", X, [Y[0], "yzero", Y[2], "yzero"]),
                ("one operand everywhere", ["x0"] * 4, ["x0"] * 4),
                ("X[0][0] == Y[0][0]", ["x0", X[1], X[2], X[3]], ["x0", Y[1], Y[2], Y[3]]),
                ("repeated pointers", ["x0", "x1", "x1", "x0"], ["y0", "y0", "y1", "y1"])]
        for label, Xn, Yn in sets:
            got = _limbs(_matmul(mp, ops, Xn, Yn, m, k, p, depth, w, ws))
            _assert_entries(got, ops.want(Xn, Yn, m, k, p), label)


@pytest.mark.parametrize("depth,w,n1,n2,head", [(8, 512, 220000, 60000, "k_pwss<18>"), (8, 512, 60000, 220000, "k_pwss<18>"),
                                                (11, 8, 300000, 30000, "k_pwm2"), (11, 8, 30000, 300000, "k_pwm2")])
def test_unbalanced_in_truncation_case_b(mp, oracle, torch_dev, depth, w, n1, n2, head):
    """X's entries run the forward side under n1's zero-row bound, Y's under n2's"""
    m, k, p = 2, 2, 2
    P = mp.dot_plan_info(k, n1, n2, depth, w)
    assert P["trunc"] > P["n"] and P["trunc"] < 2 * P["n"]
    _check_class(mp, m, k, p, n1, n2, depth, w, head)
    ops = _Ops(mp, oracle, torch_dev, n1, n2, 0xb1 + depth)
    X, Y = ["x0", "x1", "xones", "x2"], ["y0", "y1", "y2", "yones"]
    got = _limbs(_matmul(mp, ops, X, Y, m, k, p, depth, w))
    _assert_entries(got, ops.want(X, Y, m, k, p), (depth, w, n1, n2))


# ---- k_pwmm alone -----------------------------------------------------------------------------------
PLACED = [(5, 4096, None, "k_pwss<18>"), (6, 4096, None, "k_pwss<20>"), (6, 1024, "pwss", "k_pwss<10>")]
TWO_N = (0, 1)   # the residue 2^N == -1 as (limbs, top)


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


def _val(x, N):
    return x[0] + x[1] * (1 << N)


def _neg(x, N):
    """the canonical residue of p - x"""
    v = ((1 << N) + 1 - _val(x, N)) % ((1 << N) + 1)
    return (0, 1) if v == 1 << N else (v, 0)


class _Placed:
    """a (1, kk, 1) product's workspace: caches 0 .. kk-1 are X's, kk .. 2 kk - 1 are Y's"""

    def __init__(self, mp, dev, depth, w, head, kk):
        self.mp, self.dev, self.kk, self.depth, self.w = mp, dev, kk, depth, w
        self.n = n = mp.dot_max_limbs(kk, depth, w)
        P = mp.dot_plan_info(kk, n, n, depth, w)
        _check_class(mp, 1, kk, 1, n, n, depth, w, head)
        self.l, self.T, self.N = P["l"], P["trunc"], P["n"] * w
        self.ws = _mm().alloc_workspace_matmul(1, kk, 1, n, n, depth, w, dev)
        self.ws.fill_(0)
        self.views = mp.dot_workspace_views(self.ws, kk, n, n, depth, w)

    def stage(self, which, ea=(), eb=()):
        _mm().matmul_stage(which, 1, self.kk, 1, None, None, None, self.n, self.n, self.depth, self.w, self.ws, ea, eb)

    def store(self, A, B):
        """A[t], B[t]: the T residues of term t's factors -> caches t and kk + t"""
        for t in range(self.kk):
            _place(self.views, "A", self.T, A[t], self.dev)
            self.stage(_mm().STAGE_MM_STORE, [t])
            _place(self.views, "B", self.T, B[t], self.dev)
            self.stage(_mm().STAGE_MM_STORE, [self.kk + t])

    def pointwise(self, acc=False):
        import torch
        kk = self.kk
        self.stage(_mm().STAGE_MM_POINTWISE | (self.mp.STAGE_ACC if acc else 0), list(range(kk)), list(range(kk, 2 * kk)))
        torch.cuda.synchronize()
        return _read_c(self.views, self.T, self.N)

    def want(self, A, B, s):
        return _modp(sum(_val(A[t][s], self.N) * _val(B[t][s], self.N) for t in range(self.kk)), self.N)


@pytest.mark.parametrize("kk", [2, 4])
@pytest.mark.parametrize("depth,w,kind,head", PLACED)
def test_pwmm_on_placed_residues(mp, torch_dev, depth, w, kind, head, kk):
    """One term runs over every ordered pair of the eight patterns while the others are (2^N, 2^N) -- as
    term 0 and as the last term; pairs whose products cancel mod 2^N + 1; kk copies of (2^N, 2^N) and of
    (2^N, 1), which carry one sign through every term: each live slot of C against Python integers."""
    rng = random.Random(depth * 1000 + w + kk)
    with _pointwise_env(kind):
        S = _Placed(mp, torch_dev, depth, w, head, kk)
        T, N, l = S.T, S.N, S.l
        assert T >= 64
        p = (1 << N) + 1
        pats = [_pattern(q, l, N, rng) for q in range(8)]
        pa = [pats[s % 8] if s < 64 else _pattern(0, l, N, rng) for s in range(T)]
        pb = [pats[(s // 8) % 8] if s < 64 else _pattern(7, l, N, rng) for s in range(T)]
        assert len({(pa[s], pb[s]) for s in range(64)}) == 64
        fixed = [TWO_N] * T
        # cancelling pairs in terms 0 and 1, the copies of (2^N, 2^N) and (2^N, 1)
        ca = [pa[s] if s % 3 == 0 else TWO_N for s in range(T)]
        cb = [pb[s] if s % 3 == 0 else TWO_N if s % 3 == 1 else (1, 0) for s in range(T)]
        ca1 = [_neg(pa[s], N) if s % 3 == 0 else ca[s] for s in range(T)]
        rest_a = [pats[(s + 1) % 8] if s % 3 == 0 else ca[s] for s in range(T)]
        rest_b = [pats[(s + 4) % 8] if s % 3 == 0 else cb[s] for s in range(T)]
        cases = [("pairs in term 0", [pa] + [fixed] * (kk - 1), [pb] + [fixed] * (kk - 1)),
                 ("pairs in the last term", [fixed] * (kk - 1) + [pa], [fixed] * (kk - 1) + [pb]),
                 ("cancelling and same-sign terms", [ca, ca1] + [rest_a] * (kk - 2), [cb, cb] + [rest_b] * (kk - 2))]
        for label, A, B in cases:
            S.store(A, B)
            got = S.pointwise()
            bad = [s for s in range(T) if got[s] % p != S.want(A, B, s)]
            assert not bad, f"{label}: {len(bad)} of {T} slots wrong, first {bad[:8]}"
        # the cancelling slots' first two terms sum to 0 mod p: the value is the other terms' alone
        A, B = cases[2][1], cases[2][2]
        assert all((_val(A[0][s], N) * _val(B[0][s], N) + _val(A[1][s], N) * _val(B[1][s], N)) % p == 0 for s in range(0, T, 3))


def _accumulators(l, rng):
    """hand-placed reduced-form encodings (limbs, +1 carries, -1 carries, top): pending carries of both
    signs, top +-1 (the encodings of test_gpu_dot.py's last test)"""
    rnd = lambda: np.frombuffer(rng.randbytes(8 * l), dtype=np.uint64).copy()
    ones, zero = np.full(l, 2**64 - 1, np.uint64), np.zeros(l, np.uint64)
    out = []
    for top in (-1, 0, 1):
        c = [rng.choice((0, 1, -1)) for _ in range(l)]
        out.append((rnd(), {m for m in range(l) if c[m] == 1}, {m for m in range(l) if c[m] == -1}, top))
    out.append((rnd(), {l - 1}, set(), 0))
    out.append((rnd(), set(), {l - 1}, 0))
    out.append((rnd(), {l - 1}, set(), 1))
    out.append((rnd(), set(), {l - 1}, -1))
    out.append((rnd(), set(), set(), 1))
    out.append((rnd(), set(), set(), -1))
    for limbs in (ones, zero):
        out.append((limbs.copy(), set(), set(), 0))
        out.append((limbs.copy(), set(range(l)), set(), 1))
        out.append((limbs.copy(), set(), set(range(l)), -1))
        out.append((limbs.copy(), set(range(0, l, 2)), set(range(1, l, 2)), 0))
        out.append((limbs.copy(), {0, l - 1}, {l // 2}, -1))
    return out


@pytest.mark.parametrize("kk", [2, 4])
@pytest.mark.parametrize("depth,w,kind,head", PLACED)
def test_pwmm_accumulates_onto_placed_accumulators(mp, torch_dev, depth, w, kind, head, kk):
    """C hand-placed in the reduced form, then MM_POINTWISE | ACC with kk terms: (C + sum) mod 2^N + 1"""
    import torch
    rng = random.Random(depth * 77 + w + kk)
    with _pointwise_env(kind):
        S = _Placed(mp, torch_dev, depth, w, head, kk)
        T, N, l = S.T, S.N, S.l
        p = (1 << N) + 1
        accs = _accumulators(l, rng)
        digC, topC, cbC = S.views["C"]
        cbw = cbC.shape[1]
        enc = []
        for limbs, pos, neg, top in accs:
            words = stage_model.pack_masks(pos, neg, cbw)
            enc.append((limbs, top, words, stage_model.val_reduced(limbs, pos, neg, top, N)))
        hd, ht, hc = np.zeros((T, l), np.uint64), np.zeros(T, np.int32), np.zeros((T, cbw), np.uint64)
        old = []
        for s in range(T):
            hd[s], ht[s], hc[s], v = enc[s % len(accs)]
            old.append(v)
        # per slot group: every term 2^N 2^N; every term 0; random terms
        kinds = [(s // len(accs)) % 3 for s in range(T)]
        A = [[TWO_N if kinds[s] == 0 else (0, 0) if kinds[s] == 1 else _pattern(0, l, N, rng) for s in range(T)] for _ in range(kk)]
        B = [[TWO_N if kinds[s] == 0 else _pattern(0, l, N, rng) if kinds[s] == 1 else _pattern(7, l, N, rng) for s in range(T)]
             for _ in range(kk)]
        S.store(A, B)
        digC[:T] = torch.from_numpy(hd.view(np.int64)).to(torch_dev)
        topC[:T] = torch.from_numpy(ht).to(torch_dev)
        cbC[:T] = torch.from_numpy(hc.view(np.int64)).to(torch_dev)
        got = S.pointwise(acc=True)
        bad = [s for s in range(T) if got[s] % p != (old[s] + S.want(A, B, s)) % p]
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]} (encoding {[b % len(accs) for b in bad[:8]]})"


# ---- the rest ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (5, 4096, 20000), (11, 8, 5000)])
def test_stays_inside_matmul_workspace_bytes(mp, oracle, torch_dev, depth, w, n):
    """a 0xFF-filled workspace of exactly matmul_workspace_bytes with a guard region behind it"""
    import torch
    m, k, p = 2, 2, 2
    nb = _mm().matmul_workspace_bytes(m, k, p, n, n, depth, w)
    assert nb > 0
    guard = 1 << 20
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf[:nb].fill_(0xFF)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    ops = _Ops(mp, oracle, torch_dev, n, n, 0x99 + w)
    X, Y = _names(m, k, p)
    got = _limbs(_matmul(mp, ops, X, Y, m, k, p, depth, w, buf[:nb]))
    _assert_entries(got, ops.want(X, Y, m, k, p), (depth, w, n))
    assert torch.equal(buf[nb:], pat), "the product wrote past mpfft_matmul_workspace_bytes"
    ENOMEM = 4
    ptrs = (ctypes.c_void_p * 4)(*[ops.dev_of(x).data_ptr() for x in X])
    assert mp.lib().mpfft_matmul_device(ptrs, m, k, p, ptrs, ptrs, n, n, depth, w, buf.data_ptr(), nb - 1, None) == ENOMEM


@pytest.mark.parametrize("depth,w,n,kind,head", [(8, 512, 40000, None, "k_pwss<18>"), (11, 8, 5000, None, "k_pwm2")])
def test_limb_aligned_operands_and_scattered_results(mp, oracle, torch_dev, depth, w, n, kind, head):
    """operands and results starting at an odd limb of larger tensors, the results scattered over one tensor
    in another order than the matrix's"""
    import torch
    m, k, p = 2, 2, 2
    with _pointwise_env(kind):
        _check_class(mp, m, k, p, n, n, depth, w, head)
        ops = _Ops(mp, oracle, torch_dev, n, n, 0x0dd + depth)
        X, Y = _names(m, k, p)
        pad = lambda name, off: torch.cat([torch.zeros(off, dtype=torch.int64, device=torch_dev), ops.dev_of(name)])[off:]
        xs = [pad(x, 1 + 2 * i) for i, x in enumerate(X)]
        ys = [pad(y, 3 + 2 * i) for i, y in enumerate(Y)]
        assert all(t.data_ptr() % 16 == 8 for t in xs + ys)
        nr = 2 * n + 1
        blk = nr + 7   # even: every result starts at an odd limb, guard limbs between them
        big = torch.full((4 * blk + 1,), 0x77, dtype=torch.int64, device=torch_dev)
        order = [2, 0, 3, 1]
        starts = [1 + order[e] * blk for e in range(4)]
        rs = [big[s:s + nr] for s in starts]
        assert all(r.data_ptr() % 16 == 8 for r in rs)
        ws = _mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev)
        _mm().matmul_device(rs, m, k, p, xs, ys, n, n, depth, w, ws)
        got = _limbs(rs)
    _assert_entries(got, ops.want(X, Y, m, k, p), (depth, w, n))
    keep = torch.ones_like(big, dtype=torch.bool)
    for s in starts:
        keep[s:s + nr] = False
    assert (big[keep] == 0x77).all(), "a result was written outside its n1 + n2 + 1 limbs"


def test_two_streams_two_workspaces(mp, oracle, torch_dev):
    import torch
    depth, w, n, m, k, p = 8, 512, 40000, 2, 2, 2
    ops = _Ops(mp, oracle, torch_dev, n, n, 0x252)
    XA, YA = _names(m, k, p)
    XB, YB = _names(m, k, p, 8)
    for name in XA + YA + XB + YB:
        ops.dev_of(name)
    sa, sb = torch.cuda.Stream(device=torch_dev), torch.cuda.Stream(device=torch_dev)
    wa, wb = (_mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev) for _ in range(2))
    ra, rb = ([torch.zeros(2 * n + 1, dtype=torch.int64, device=torch_dev) for _ in range(4)] for _ in range(2))
    torch.cuda.synchronize()
    for _ in range(2):
        _matmul(mp, ops, XA, YA, m, k, p, depth, w, wa, sa, ra)
        _matmul(mp, ops, XB, YB, m, k, p, depth, w, wb, sb, rb)
    sa.synchronize()
    sb.synchronize()
    _assert_entries(_limbs(ra), ops.want(XA, YA, m, k, p), "stream a")
    _assert_entries(_limbs(rb), ops.want(XB, YB, m, k, p), "stream b")


@pytest.mark.parametrize("m,k,p,n1,n2", [(1, 1, 1, 1, 1), (2, 3, 2, 7, 5), (2, 2, 2, 1000, 900), (2, 2, 1, 100000, 100000),
                                         (2, 2, 2, 600000, 600000)])
def test_host_entries(mp, oracle, m, k, p, n1, n2):
    xs = [mp.fill_random(n1, 0xabc + n1 + i) for i in range(m * k)]
    ys = [mp.fill_random(n2, 0xdef + n2 + i) for i in range(k * p)]
    want = [from_int(sum(to_int(oracle.gmp_mul(xs[i * k + t], ys[t * p + j])) for t in range(k)), n1 + n2 + 1)
            for i in range(m) for j in range(p)]
    depth, w = mp.dot_choose(k, n1, n2)
    _assert_entries(_mm().matmul(xs, ys, m, k, p, depth, w), want, (m, k, p, n1, n2, depth, w))
    _assert_entries(_mm().matmul_auto([xs[i * k:(i + 1) * k] for i in range(m)], [ys[t * p:(t + 1) * p] for t in range(k)], m, k, p),
                    want, (m, k, p, n1, n2))


def test_profile_covers_matrix_products(mp, oracle, torch_dev):
    """seven stage times; every matrix entry and every result entry claims a call slot"""
    depth, w, n, m, k, p = 8, 512, 40000, 2, 2, 1
    ops = _Ops(mp, oracle, torch_dev, n, n, 0x321)
    X, Y = _names(m, k, p)
    ws = _mm().alloc_workspace_matmul(m, k, p, n, n, depth, w, torch_dev)
    for name in X + Y:
        ops.dev_of(name)
    mp.profile_begin(m * k + k * p + m * p)
    rs = _matmul(mp, ops, X, Y, m, k, p, depth, w, ws)
    got = _limbs(rs)
    ms, calls = mp.profile_end()
    assert calls == m * k + k * p + m * p
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert ms["pointwise"] > 0 and ms["fwd_columns"] > 0 and ms["fwd_rows"] > 0 and ms["inv_rows"] > 0, ms
    _assert_entries(got, ops.want(X, Y, m, k, p), "profiled")


def test_c_caller_matmul(mp):
    exe = os.path.join(HERE, "c_matmul", "matmul_caller")
    assert os.path.exists(exe), "tests/c_matmul/matmul_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
