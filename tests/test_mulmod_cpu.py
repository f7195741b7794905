"""CPU-only checks of the products mod 2^B + 1 (mpfft_mulmod_*, include/mpfft.h): no
device is touched.

- the arithmetic contract in Python integers: pieces with the top limb folded into piece 0, the
  weight theta^j, the cyclic product mod p, un-weight and scaling, the sign read back from the
  canonical residue, the signed sum mod M -- against a * b % M, with the coefficient bound
- parameter validation, the chooser and the size rounding, workspace sizes, kernel names
"""
import random

import pytest

from helpers import chunks
from stage_model import modp

EINVAL, ETOOBIG, EUNSUPPORTED = 1, 2, 3

# (depth, w, L): each at the largest bits1 its (depth, w) allows
SHAPES = [(4, 4, 14), (4, 8, 30), (5, 2, 28), (6, 64, 4088), (6, 192, 12280), (6, 512, 32760),
          (5, 1024, 16380), (5, 2048, 32764), (5, 4096, 65532)]
IDS = ["d%d-w%d-L%d" % s for s in SHAPES]


def full_L(depth, w):
    """the largest L of (depth, w): bits1 <= (N - depth - 2) / 2 with 2n bits1 a multiple of 64"""
    n = 1 << depth
    b = (n * w - depth - 2) // 2
    while (2 * n * b) % 64:
        b -= 1
    return 2 * n * b // 64


def operand_pairs(B, rng):
    M = (1 << B) + 1
    return [(M - 1, M - 1), (M - 1, 1), (M - 2, M - 2), ((1 << B) - 1, (1 << B) - 1), (2, 1 << (B - 1)), (0, 5),
            (rng.randrange(M), rng.randrange(M)), (rng.randrange(M), rng.randrange(1 << 64))]


def pieces(a, B, n2, b1):
    """x_j: the bits1-bit pieces of the low B bits; the top limb enters piece 0 negated (2^B == -1)"""
    x = chunks(a & ((1 << B) - 1), n2, b1)
    x[0] -= a >> B
    return x


def negacyclic(x, y, S):
    """signed c_k = sum_{i+j=k} x_i y_j - sum_{i+j=k+len} x_i y_j, through one product of the
    sequences packed S bits apart (|coefficient of the plain product| < 2^(S-1))"""
    m = len(x)
    X = sum(v << (j * S) for j, v in enumerate(x))
    Y = sum(v << (j * S) for j, v in enumerate(y))
    half = 1 << (S - 1)
    P = X * Y + sum(half << (k * S) for k in range(2 * m))   # every digit made non-negative
    mask = (1 << S) - 1
    d = [((P >> (k * S)) & mask) - half for k in range(2 * m)]
    return [d[k] - d[k + m] for k in range(m)]


def theta_of(depth, w):
    N = (1 << depth) * w
    p = (1 << N) + 1
    if w % 2 == 0:
        return pow(2, w // 2, p)
    sqrt2 = ((1 << (3 * N // 4)) - (1 << (N // 4))) % p
    return pow(sqrt2, w, p)


def read_back(cs, N, b1, M):
    """canonical residues -> signed coefficients -> sum c_j 2^(j bits1) mod M"""
    p = (1 << N) + 1
    signed = [c - p if 2 * c > p else c for c in cs]
    return signed, sum(c << (j * b1) for j, c in enumerate(signed)) % M


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_contract_in_python_integers(depth, w, L):
    """split, signed negacyclic product, canonical residues mod p, sign read-back, sum mod M"""
    assert L == full_L(depth, w)
    n, B = 1 << depth, 64 * L
    N, n2 = n * w, 2 * n
    b1 = B // n2
    assert b1 * n2 == B and 2 * b1 + depth + 2 <= N
    p, M = (1 << N) + 1, (1 << B) + 1
    rng = random.Random(L)
    for a, b in operand_pairs(B, rng):
        c = negacyclic(pieces(a, B, n2, b1), pieces(b, B, n2, b1), 2 * b1 + depth + 4)
        assert max(abs(v) for v in c) < 1 << (N - 1)
        assert max(abs(v) for v in c) < n2 << (2 * b1)
        signed, r = read_back([v % p for v in c], N, b1, M)
        assert signed == c
        assert r == modp(a * b, B)   # a * b % M by folding at 2^B == -1
        assert 0 <= r <= 1 << B


@pytest.mark.parametrize("depth,w,L", SHAPES[:4] + [(6, 1, 56), (5, 6, 42)],
                         ids=IDS[:4] + ["d6-w1-L56-sqrt2", "d5-w6-L42"])
def test_weighted_cyclic_product_is_the_contract(depth, w, L):
    """the transform route itself: X_j = theta^j x_j, cyclic product mod p, theta^-j 2^-(depth+1)
    (the cyclic product here is the plain one; the library's transforms leave 2^(depth+1) times it)"""
    n, B = 1 << depth, 64 * L
    N, n2 = n * w, 2 * n
    b1 = B // n2
    assert b1 * n2 == B and 2 * b1 + depth + 2 <= N
    p, M = (1 << N) + 1, (1 << B) + 1
    th = theta_of(depth, w)
    assert pow(th, n2, p) == p - 1 and pow(th, 2 * n2, p) == 1   # a primitive 4n-th root of unity
    thj = [pow(th, j, p) for j in range(n2)]
    inv = [pow(th, 2 * n2 - j, p) for j in range(n2)]
    rng = random.Random(L + 1)
    for a, b in operand_pairs(B, rng):
        X = [t * v % p for t, v in zip(thj, pieces(a, B, n2, b1))]
        Y = [t * v % p for t, v in zip(thj, pieces(b, B, n2, b1))]
        Z = [sum(X[i] * Y[(k - i) % n2] for i in range(n2)) % p for k in range(n2)]
        signed, r = read_back([z * t % p for z, t in zip(Z, inv)], N, b1, M)
        assert max(abs(v) for v in signed) < 1 << (N - 1)
        assert r == modp(a * b, B)


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_check_params_accepts(mp, depth, w, L):
    assert mp.mulmod_check_params(L, depth, w) == 0
    P = mp.mulmod_plan_info(L, depth, w)
    n = 1 << depth
    assert (P["n"], P["l"], P["trunc"], P["bits1"]) == (n, n * w // 64, 2 * n, 64 * L // (2 * n))
    assert P["NC"] * P["NR"] == 2 * n and P["j1"] == P["j2"] == 2 * n


def test_check_params_rejects(mp):
    assert mp.mulmod_check_params(4087, 6, 64) == EINVAL          # 2n = 128 does not divide 64 L
    assert mp.mulmod_check_params(0, 6, 64) == EINVAL
    assert mp.mulmod_check_params(14, 1, 32) == EINVAL            # depth 1
    assert mp.mulmod_check_params(14, 4, 3) == EINVAL             # N = 48: not whole limbs
    assert mp.mulmod_check_params(1000, 7, 4096) == EUNSUPPORTED  # l = 8192
    for depth, w, L in SHAPES:                                    # bits1 one step too large
        g = max(1, (2 << depth) // 64)
        assert mp.mulmod_check_params(L + g, depth, w) == ETOOBIG, (depth, w, L)
        assert mp.mulmod_workspace_bytes(L + g, depth, w) == 0
    with pytest.raises(mp.MpfftError):
        mp.mulmod_plan_info(15, 4, 4)
    with pytest.raises(mp.MpfftError):
        mp.mulmod_stage_kernels(15, 4, 4)


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_choose_is_valid(mp, depth, w, L):
    d, wv = mp.mulmod_choose(L)
    assert mp.mulmod_check_params(L, d, wv) == 0
    assert wv & (wv - 1) == 0


@pytest.mark.parametrize("m", [1, 1000, 10 ** 6, 33550336])
def test_next_size(mp, m):
    L, d, wv = mp.mulmod_next_size(m)
    assert L >= m and mp.mulmod_check_params(L, d, wv) == 0
    if m == 33550336:   # the full-efficiency size of (14, 8): nothing to round
        assert m == full_L(14, 8)
        assert (L, d, wv) == (m, 14, 8)


def test_next_size_rejects(mp):
    with pytest.raises(mp.MpfftError):
        mp.mulmod_next_size(0)
    with pytest.raises(mp.MpfftError):
        mp.mulmod_choose(1 << 40)   # no supported pair holds it


def test_workspace_bytes(mp):
    for depth, w, L in SHAPES + [(14, 8, 33550336)]:
        mul, sq = mp.mulmod_workspace_bytes(L, depth, w), mp.mulmod_workspace_bytes(L, depth, w, True)
        assert 0 < sq < mul, (depth, w, L)
        lay, ls = mp.mulmod_workspace_layout(L, depth, w), mp.mulmod_workspace_layout(L, depth, w, True)
        assert (ls["digB"], ls["topB"], ls["cbB"]) == (0, 0, 0) and lay["digB"] > 0
        assert lay["slots"] == ls["slots"] == 2 << depth
    L = 33550336
    assert mp.mulmod_workspace_bytes(L, 14, 8) < mp.workspace_bytes(L, L, *mp.choose(L, L))


@pytest.mark.parametrize("depth,w,L", SHAPES + [(14, 8, 33550336), (6, 3, 184), (9, 256, 1048480)],
                         ids=IDS + ["d14-w8", "d6-w3-odd", "d9-w256"])
def test_stage_kernels_name_every_stage(mp, depth, w, L):
    for sqr in (False, True):
        k = mp.mulmod_stage_kernels(L, depth, w, sqr)
        assert set(k) == set(mp.STAGE_NAMES)
        assert all(v.strip() for v in k.values()), k
        assert k["fwd_columns"].startswith("k_nweight<")
        assert "k_nwrap" in k["combine"] and "k_nfix" in k["combine"] and "k_combine1" in k["combine"]
        l = (1 << depth) * w // 64
        if l in (1024, 2048, 4096) and w % 2 == 0:
            assert k["scale"].startswith("k_rscale")
        else:
            assert k["scale"].startswith("k_nunweight<")
        if sqr:
            assert k["pointwise"].startswith("k_pwsq") or k["pointwise"].endswith("(B = A)")


def test_version_has_the_mulmod_entries(mp):
    assert mp.lib().mpfft_version() >= 4
