"""CPU-only checks of the products mod 2^B + 1 with the low-word CRT (mpfft_mulmodw_*,
include/mpfft.h): no device is touched.

- the arithmetic contract in Python integers: pieces with the top limb folded into piece 0, the
  signed negacyclic product c, its canonical residue c~ mod p, the negacyclic convolution d of the
  pieces' low words mod 2^32, t = (d - c~) mod 2^32 read as a signed int32, c~ + t p == c, and the
  signed sum mod M against a * b % M -- at shapes past the plain family's bound
- parameter validation, the chooser and the size rounding, workspace sizes, kernel names, and the
  plain family's recorded answers (tests/golden/mulmod_answers.json) once more
"""
import json
import os
import random

import pytest

from helpers import chunks
from stage_model import modp

EINVAL, ETOOBIG, EUNSUPPORTED = 1, 2, 3


def full_Lw(depth, w):
    """the largest L of (depth, w) here: bits1 <= (N + 32 - depth - 2) / 2 with 2n bits1 a multiple of 64"""
    n = 1 << depth
    b = (n * w + 32 - depth - 2) // 2
    while (2 * n * b) % 64:
        b -= 1
    return 2 * n * b // 64


# (depth, w, L): the Fermat shape (bits1 = N / 2 = 64), an odd bits1 = 75 (the low words straddle
# limbs), then each (depth, w) at the largest bits1 the bound allows -- (4, 8, 38): bits1 = 76 > N / 2
SHAPES = [(4, 8, 32), (5, 4, 75), (4, 8, 38), (5, 4, 76), (2, 16, 5), (6, 1, 88), (6, 64, 4120),
          (5, 2048, 32780), (5, 4096, 65548)]
FULL = SHAPES[2:]
IDS = ["d%d-w%d-L%d" % s for s in SHAPES]


def operand_pairs(B, rng):
    M = (1 << B) + 1
    return [(M - 1, M - 1), (M - 1, 1), (M - 2, M - 2), ((1 << B) - 1, (1 << B) - 1), (2, 1 << (B - 1)), (0, 5),
            (M - 1, (1 << B) - 1), (rng.randrange(M), rng.randrange(M)), (rng.randrange(M), rng.randrange(1 << 64))]


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


def lowconv(x, y):
    """the negacyclic convolution of the low words x_j mod 2^32, y_j mod 2^32, in arithmetic mod 2^32"""
    m, W = len(x), 1 << 32
    xl, yl = [v % W for v in x], [v % W for v in y]
    return [v % W for v in negacyclic(xl, yl, 64 + m.bit_length() + 2)]


def int32(v):
    v %= 1 << 32
    return v - (1 << 32) if v >> 31 else v


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_contract_in_python_integers(depth, w, L):
    """pieces, c, c~ = c mod p, d = the low-word convolution, t, c~ + t p == c, the sum mod M"""
    if (depth, w, L) in FULL:
        assert L == full_Lw(depth, w)
    n, B = 1 << depth, 64 * L
    N, n2 = n * w, 2 * n
    b1 = B // n2
    assert b1 * n2 == B and b1 >= 32
    assert 2 * b1 + depth + 2 > N          # the plain family's bound fails
    assert 2 * b1 + depth + 2 <= N + 32    # this one holds
    p, M = (1 << N) + 1, (1 << B) + 1
    assert p % (1 << 32) == 1
    rng = random.Random(L)
    tmax = 0
    for a, b in operand_pairs(B, rng):
        x, y = pieces(a, B, n2, b1), pieces(b, B, n2, b1)
        c = negacyclic(x, y, 2 * b1 + depth + 4)
        assert max(abs(v) for v in c) < n2 << (2 * b1)
        assert max(abs(v) for v in c) < 1 << (N + 31)
        ct = [v % p for v in c]
        d = lowconv(x, y)
        assert d == [v % (1 << 32) for v in c]
        t = [int32(dk - ck) for dk, ck in zip(d, ct)]
        assert t == [v // p for v in c]
        assert [ck + tk * p for ck, tk in zip(ct, t)] == c
        r = sum(v << (j * b1) for j, v in enumerate(c)) % M
        assert r == modp(a * b, B)   # a * b % M by folding at 2^B == -1
        assert 0 <= r <= 1 << B
        tmax = max(tmax, max(abs(v) for v in t))
    assert tmax >= n, tmax   # the CRT step does work: reading the sign alone (t in {0, -1}) would fail
    if (depth, w, L) == (4, 8, 38):
        assert tmax >= 1 << 28, tmax


def test_low_word_of_the_top_limb():
    """x_0 = -1 (the operand 2^B) contributes 0xFFFFFFFF to the low-word convolution"""
    B, n2, b1 = 64 * 32, 32, 64
    x = pieces(1 << B, B, n2, b1)
    assert x[0] == -1 and not any(x[1:])
    y = pieces(5, B, n2, b1)
    assert lowconv(x, y)[0] == (-5) % (1 << 32)


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_check_params_accepts(mp, depth, w, L):
    assert mp.mulmodw_check_params(L, depth, w) == 0
    assert mp.mulmod_check_params(L, depth, w) == ETOOBIG
    P = mp.mulmodw_plan_info(L, depth, w)
    n = 1 << depth
    assert (P["n"], P["l"], P["trunc"], P["bits1"]) == (n, n * w // 64, 2 * n, 64 * L // (2 * n))
    assert P["NC"] * P["NR"] == 2 * n and P["j1"] == P["j2"] == 2 * n


def test_check_params_rejects(mp):
    assert mp.mulmodw_check_params(4119, 6, 64) == EINVAL          # 2n = 128 does not divide 64 L
    assert mp.mulmodw_check_params(0, 6, 64) == EINVAL
    assert mp.mulmodw_check_params(32, 1, 32) == EINVAL            # depth 1
    assert mp.mulmodw_check_params(14, 4, 3) == EINVAL             # N = 48: not whole limbs
    assert mp.mulmodw_check_params(14, 4, 4) == EINVAL             # bits1 = 28 < 32 (valid in the plain family)
    assert mp.mulmod_check_params(14, 4, 4) == 0
    assert mp.mulmodw_check_params(62, 6, 64) == EINVAL            # bits1 = 31
    assert mp.mulmodw_check_params(64, 6, 64) == 0                 # bits1 = 32
    assert mp.mulmodw_workspace_bytes(14, 4, 4) == 0
    assert mp.mulmodw_check_params(1000, 7, 4096) == EUNSUPPORTED  # l = 8192
    for depth, w, L in FULL:                                       # bits1 one step too large
        g = max(1, (2 << depth) // 64)
        assert mp.mulmodw_check_params(L + g, depth, w) == ETOOBIG, (depth, w, L)
        assert mp.mulmodw_workspace_bytes(L + g, depth, w) == 0
        assert mp.mulmodw_workspace_bytes(L + g, depth, w, True) == 0
    with pytest.raises(mp.MpfftError):
        mp.mulmodw_plan_info(39, 4, 8)
    with pytest.raises(mp.MpfftError):
        mp.mulmodw_stage_kernels(39, 4, 8)
    with pytest.raises(mp.MpfftError):
        mp.mulmodw_workspace_layout(39, 4, 8)


def test_every_plain_shape_from_bits1_32_on_is_valid_here(mp):
    """what mulmod_check_params accepts, this family accepts too once bits1 >= 32, with the same plan"""
    seen = 0
    for depth in range(2, 12):
        for w in (1, 2, 4, 8, 16, 64, 256, 1024, 4096):
            n = 1 << depth
            if (n * w) % 64 or n * w // 64 > 4096:
                continue
            g = max(1, 2 * n // 64)
            for b1 in (31, 32, 33, n * w // 4, (n * w - depth - 2) // 2):
                L = 2 * n * b1 // 64 // g * g
                if L < 1 or mp.mulmod_check_params(L, depth, w):
                    continue
                want = 0 if 64 * L // (2 * n) >= 32 else EINVAL
                assert mp.mulmodw_check_params(L, depth, w) == want, (depth, w, L)
                if want == 0:
                    assert mp.mulmodw_plan_info(L, depth, w) == mp.mulmod_plan_info(L, depth, w)
                    seen += 1
    assert seen > 50


@pytest.mark.parametrize("L", [4, 5, 38, 1000, 1 << 10, 1 << 16, 1 << 20, 1 << 24, 33550336])
def test_choose_is_valid(mp, L):
    d, wv = mp.mulmodw_choose(L)
    assert mp.mulmodw_check_params(L, d, wv) == 0
    assert wv & (wv - 1) == 0


@pytest.mark.parametrize("k", range(10, 25))
def test_choose_halves_the_transform_at_power_of_two_sizes(mp, k):
    """L = 2^k: bits1 = B / 2n and N are powers of two, so the plain bound 2 bits1 + depth + 2 <= N
    allows bits1 <= N / 4 only and every plain candidate has N 2n >= 4 B; here bits1 = N / 2 is valid
    (N + depth + 2 <= N + 32), N 2n = 2 B.  The chooser minimises predicted time, not size: what must
    hold is that its pick is no larger than the plain family's."""
    L = 1 << k
    B = 64 * L
    d0, w0 = mp.mulmod_choose(L)
    d1, w1 = mp.mulmodw_choose(L)
    size0, size1 = (w0 << d0) * (2 << d0), (w1 << d1) * (2 << d1)
    assert size0 >= 4 * B and size1 >= 2 * B
    assert size1 <= size0, (L, (d0, w0), (d1, w1))


@pytest.mark.parametrize("m", [1, 3, 1000, 10 ** 6, 1 << 24])
def test_next_size(mp, m):
    L, d, wv = mp.mulmodw_next_size(m)
    assert L >= m and mp.mulmodw_check_params(L, d, wv) == 0
    assert L < 2 * m + 8


def test_next_size_rejects(mp):
    with pytest.raises(mp.MpfftError):
        mp.mulmodw_next_size(0)
    with pytest.raises(mp.MpfftError) as e:
        mp.mulmodw_choose(3)         # 2n = 8 pieces of 24 bits: no bits1 >= 32
    assert e.value.code == EINVAL
    with pytest.raises(mp.MpfftError):
        mp.mulmodw_choose(1 << 40)   # no supported pair holds it


def test_workspace_bytes_and_layout(mp):
    for depth, w, L in SHAPES + [(14, 4, 1 << 24)]:
        mul, sq = mp.mulmodw_workspace_bytes(L, depth, w), mp.mulmodw_workspace_bytes(L, depth, w, True)
        assert 0 < sq < mul, (depth, w, L)
        lay, ls = mp.mulmodw_workspace_layout(L, depth, w), mp.mulmodw_workspace_layout(L, depth, w, True)
        assert (ls["digB"], ls["topB"], ls["cbB"]) == (0, 0, 0) and lay["digB"] > 0
        assert lay["slots"] == ls["slots"] == 2 << depth
        for la, nb in ((lay, mul), (ls, sq)):   # d: 2n uint32 behind everything else
            assert la["d"] % 4 == 0 and la["d"] + 4 * (2 << depth) <= nb < la["d"] + 4 * (2 << depth) + 256
    # where both families are valid the regions in front of d are the plain family's
    depth, w, L = 6, 64, 4088
    a, b = mp.mulmod_workspace_layout(L, depth, w), mp.mulmodw_workspace_layout(L, depth, w)
    assert all(a[k] == b[k] for k in a)
    assert b["d"] == mp.mulmod_workspace_bytes(L, depth, w)
    L = 1 << 24   # the Fermat size: half the plain family's workspace, near enough
    assert mp.mulmodw_workspace_bytes(L, *mp.mulmodw_choose(L)) < 0.6 * mp.mulmod_workspace_bytes(L, *mp.mulmod_choose(L))


@pytest.mark.parametrize("depth,w,L", SHAPES + [(14, 4, 1 << 24), (6, 3, 216), (9, 256, 1048576)],
                         ids=IDS + ["d14-w4", "d6-w3-odd", "d9-w256"])
def test_stage_kernels_name_every_stage(mp, depth, w, L):
    for sqr in (False, True):
        k = mp.mulmodw_stage_kernels(L, depth, w, sqr)
        assert set(k) == set(mp.STAGE_NAMES)
        assert all(v.strip() for v in k.values()), k
        assert k["fwd_columns"].startswith("k_nweight<")
        for name in ("k_nlowconv", "k_combine1", "k_nwrapw", "k_nfix"):
            assert name in k["combine"], k
        l = (1 << depth) * w // 64
        if l in (1024, 2048, 4096) and w % 2 == 0:
            assert k["scale"].startswith("k_rscale")
        else:
            assert k["scale"].startswith("k_nunweight<")
        if sqr:
            assert k["pointwise"].startswith("k_pwsq") or k["pointwise"].endswith("(B = A)")
    plain = mp.mulmod_stage_kernels(4088, 6, 64)["combine"]
    assert "k_nwrapw" not in plain and "k_nlowconv" not in plain


def test_version_has_the_mulmodw_entries(mp):
    assert mp.lib().mpfft_version() >= 7
    for name in ("mpfft_mulmodw_check_params", "mpfft_mulmodw_ex", "mpfft_sqrmodw_ex", "mpfft_mulmodw_device",
                 "mpfft_sqrmodw_device", "mpfft_mulmodw_workspace_bytes", "mpfft_mulmodw_plan_info",
                 "mpfft_mulmodw_workspace_layout", "mpfft_mulmodw_stage", "mpfft_mulmodw_stage_kernels",
                 "mpfft_mulmodw_choose", "mpfft_mulmodw_next_size"):
        assert hasattr(mp.lib(), name), name
    assert mp.STAGE_LOWCONV == 9


def test_every_existing_mulmod_answer_is_unchanged(mp):
    """the plain mod 2^B + 1 entries against the answers recorded before this family existed"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mulmod_answers.json")) as f:
        rec = json.load(f)
    for e in rec["shapes"]:
        d, w, L = e["depth"], e["w"], e["L"]
        assert mp.mulmod_check_params(L, d, w) == e["check"], (d, w, L)
        assert [mp.mulmod_workspace_bytes(L, d, w, s) for s in (False, True)] == e["ws"], (d, w, L)
        if e["check"] == 0:
            assert mp.mulmod_plan_info(L, d, w) == e["plan"], (d, w, L)
            assert [mp.mulmod_workspace_layout(L, d, w, s) for s in (False, True)] == e["layout"], (d, w, L)
            assert [mp.mulmod_stage_kernels(L, d, w, s) for s in (False, True)] == e["kernels"], (d, w, L)
    for L, want in rec["choose"]:
        assert list(mp.mulmod_choose(L)) == want, L
    for L, want in rec["next_size"]:
        assert list(mp.mulmod_next_size(L)) == want, L
