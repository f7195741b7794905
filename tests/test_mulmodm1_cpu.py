"""CPU-only checks of the products mod 2^B - 1 (mpfft_mulmodm1_*, include/mpfft.h): no
device is touched.

- the arithmetic contract in Python integers: unweighted pieces, the cyclic convolution, the
  coefficient bound 2 bits1 + depth + 1 <= N, the sum mod M, fully reduced -- against a * b % M
- parameter validation, the chooser and the size rounding, workspace sizes, kernel names
- the answers of the mod 2^B + 1 entries are those recorded from the library before the cyclic
  entries were added (tests/golden/mulmod_answers.json)
"""
import json
import os
import random

import pytest

from helpers import chunks

EINVAL, ETOOBIG, EUNSUPPORTED = 1, 2, 3
MUL, SQR, PRE = 0, 1, 2

# (depth, w, L): the shapes the contract was stated on, most at the cyclic full size
SHAPES = [(4, 4, 14), (4, 8, 30), (5, 64, 1021), (6, 64, 4088), (6, 1, 56), (6, 3, 184), (4, 4, 7), (6, 64, 2048),
          (2, 16, 1), (2, 32, 1)]
IDS = ["d%d-w%d-L%d" % s for s in SHAPES]
# each at the largest bits1 its (depth, w) allows
FULL = [(4, 4, 14), (4, 8, 30), (5, 64, 1021), (6, 64, 4088), (6, 1, 56), (6, 3, 184), (6, 192, 12280), (6, 512, 32760),
        (5, 1024, 16381), (5, 2048, 32765), (5, 4096, 65533), (14, 8, 33550336)]


def full_L(depth, w):
    """the largest L of (depth, w): bits1 <= (N - depth - 1) / 2 with 2n bits1 a multiple of 64"""
    n = 1 << depth
    b = (n * w - depth - 1) // 2
    while (2 * n * b) % 64:
        b -= 1
    return 2 * n * b // 64


def operand_pairs(B, rng):
    M = (1 << B) - 1
    return [(M, M), (M, rng.randrange(M)), (M - 1, M - 1), (2, 1 << (B - 1)), (1, rng.randrange(M)), (0, 5),
            (rng.randrange(M + 1), rng.randrange(M + 1)), (rng.randrange(M + 1), rng.randrange(1 << min(B, 64)))]


def cyclic(x, y, S):
    """c_k = sum_{i+j == k mod len} x_i y_j through one product of the sequences packed S bits apart"""
    m = len(x)
    X = sum(v << (j * S) for j, v in enumerate(x))
    Y = sum(v << (j * S) for j, v in enumerate(y))
    d = chunks(X * Y, 2 * m, S)
    return [d[k] + d[k + m] for k in range(m)]


@pytest.mark.parametrize("depth,w,L", SHAPES, ids=IDS)
def test_contract_in_python_integers(depth, w, L):
    """pieces (the last one ends exactly at bit B), cyclic convolution, bound, sum mod M"""
    n, B = 1 << depth, 64 * L
    N, n2 = n * w, 2 * n
    b1 = B // n2
    assert b1 * n2 == B and 2 * b1 + depth + 1 <= N
    M = (1 << B) - 1
    rng = random.Random(L)
    for a, b in operand_pairs(B, rng):
        x, y = chunks(a, n2, b1), chunks(b, n2, b1)
        assert sum(v << (j * b1) for j, v in enumerate(x)) == a
        c = cyclic(x, y, 2 * b1 + depth + 2)
        assert 0 <= min(c) and max(c) <= n2 * ((1 << b1) - 1) ** 2 < 1 << N   # canonical: the carry limb is never set
        r = sum(v << (j * b1) for j, v in enumerate(c)) % M
        assert r == a * b % M and 0 <= r < M


@pytest.mark.parametrize("depth,w,L", [(4, 4, 14), (5, 2, 28), (6, 1, 56), (6, 3, 184), (2, 16, 1)],
                         ids=["d4-w4-L14", "d5-w2-L28", "d6-w1-L56", "d6-w3-L184", "d2-w16-L1"])
def test_transform_route_is_the_contract(depth, w, L):
    """the route itself: the length-2n transform with root 2^w mod p = 2^N + 1 of the unweighted
    pieces, pointwise products, inverse and 2^-(depth+1) -- odd w included, no sqrt2 anywhere"""
    n, B = 1 << depth, 64 * L
    N, n2 = n * w, 2 * n
    b1 = B // n2
    p, M = (1 << N) + 1, (1 << B) - 1
    root = pow(2, w, p)
    assert pow(root, n, p) == p - 1   # a primitive 2n-th root of unity
    dft = lambda v, g: [sum(vj * pow(g, j * k, p) for j, vj in enumerate(v)) % p for k in range(n2)]
    rng = random.Random(L + 2)
    for a, b in operand_pairs(B, rng)[:5]:
        X, Y = dft(chunks(a, n2, b1), root), dft(chunks(b, n2, b1), root)
        Z = dft([u * v % p for u, v in zip(X, Y)], pow(root, n2 - 1, p))
        c = [z * pow(2, 2 * N - depth - 1, p) % p for z in Z]
        assert c == cyclic(chunks(a, n2, b1), chunks(b, n2, b1), 2 * b1 + depth + 2)
        assert sum(v << (j * b1) for j, v in enumerate(c)) % M == a * b % M


@pytest.mark.parametrize("depth,w,L", SHAPES + FULL[6:], ids=IDS + ["d%d-w%d-L%d" % s for s in FULL[6:]])
def test_check_params_accepts(mp, depth, w, L):
    assert mp.mulmodm1_check_params(L, depth, w) == 0
    P = mp.mulmodm1_plan_info(L, depth, w)
    n = 1 << depth
    assert (P["n"], P["l"], P["trunc"], P["bits1"]) == (n, n * w // 64, 2 * n, 64 * L // (2 * n))
    assert P["NC"] * P["NR"] == 2 * n and P["j1"] == P["j2"] == 2 * n


def test_check_params_rejects(mp):
    assert mp.mulmodm1_check_params(4087, 6, 64) == EINVAL          # 2n = 128 does not divide 64 L
    assert mp.mulmodm1_check_params(0, 6, 64) == EINVAL
    assert mp.mulmodm1_check_params(14, 1, 32) == EINVAL            # depth 1
    assert mp.mulmodm1_check_params(14, 31, 1) == EINVAL            # depth 31
    assert mp.mulmodm1_check_params(14, 4, 3) == EINVAL             # N = 48: not whole limbs
    assert mp.mulmodm1_check_params(1000, 7, 4096) == EUNSUPPORTED  # l = 8192
    for depth, w, L in FULL:                                        # bits1 one granularity step too large
        assert L == full_L(depth, w)
        g = max(1, (2 << depth) // 64)
        assert mp.mulmodm1_check_params(L + g, depth, w) == ETOOBIG, (depth, w, L)
        for kind in (MUL, SQR, PRE):
            assert mp.mulmodm1_workspace_bytes(L + g, depth, w, kind) == 0
        assert mp.mulmodm1_precomp_bytes(L + g, depth, w) == 0
    assert mp.mulmodm1_workspace_bytes(14, 4, 4, 3) == 0            # no such kind
    with pytest.raises(mp.MpfftError):
        mp.mulmodm1_plan_info(15, 4, 4)
    with pytest.raises(mp.MpfftError):
        mp.mulmodm1_stage_kernels(15, 4, 4)


def test_one_bit_more_room_than_the_negacyclic_bound(mp):
    """2 bits1 + depth + 1 <= N against 2 bits1 + depth + 2 <= N: (5, 64, 1021) is valid here only"""
    assert mp.mulmodm1_check_params(1021, 5, 64) == 0
    assert mp.mulmod_check_params(1021, 5, 64) == ETOOBIG


@pytest.mark.parametrize("depth,w,L", SHAPES + FULL[6:], ids=IDS + ["d%d-w%d-L%d" % s for s in FULL[6:]])
def test_choose_is_valid(mp, depth, w, L):
    d, wv = mp.mulmodm1_choose(L)
    assert mp.mulmodm1_check_params(L, d, wv) == 0
    assert wv & (wv - 1) == 0


@pytest.mark.parametrize("m", [1, 1000, 5000, 10 ** 6, 33550336])
def test_next_size(mp, m):
    L, d, wv = mp.mulmodm1_next_size(m)
    assert L >= m and mp.mulmodm1_check_params(L, d, wv) == 0
    if m == 33550336:   # the full-efficiency size of (14, 8): nothing to round
        assert m == full_L(14, 8)
        assert (L, d, wv) == (33550336, 14, 8)


def test_next_size_rejects(mp):
    with pytest.raises(mp.MpfftError):
        mp.mulmodm1_next_size(0)
    with pytest.raises(mp.MpfftError):
        mp.mulmodm1_choose(1 << 40)   # no supported pair holds it


def test_workspace_bytes(mp):
    for depth, w, L in SHAPES + FULL[6:]:
        mul, sq, pre = (mp.mulmodm1_workspace_bytes(L, depth, w, k) for k in (MUL, SQR, PRE))
        assert 0 < sq < mul and pre == sq, (depth, w, L)
        assert mp.mulmodm1_precomp_bytes(L, depth, w) > 0
        lay = mp.mulmodm1_workspace_layout(L, depth, w)
        assert lay["digB"] > 0
        for k in (SQR, PRE):
            ls = mp.mulmodm1_workspace_layout(L, depth, w, k)
            assert (ls["digB"], ls["topB"], ls["cbB"]) == (0, 0, 0)
            assert lay["slots"] == ls["slots"] == 2 << depth
    L = 33550336
    assert mp.mulmodm1_workspace_bytes(L, 14, 8) < mp.workspace_bytes(L, L, *mp.choose(L, L))


@pytest.mark.parametrize("depth,w,L", SHAPES + FULL[6:] + [(9, 256, 1048496), (8, 1024, 1048536)],
                         ids=IDS + ["d%d-w%d-L%d" % s for s in FULL[6:]] + ["d9-w256", "d8-w1024"])
def test_stage_kernels_name_every_stage(mp, depth, w, L):
    l = (1 << depth) * w // 64
    for kind in (MUL, SQR, PRE):
        k = mp.mulmodm1_stage_kernels(L, depth, w, kind)
        assert set(k) == set(mp.STAGE_NAMES)
        assert all(v.strip() for v in k.values()), k
        assert "split" in k["fwd_columns"] and "k_nweight" not in k["fwd_columns"]
        if l in (1024, 2048, 4096):
            assert k["fwd_columns"].startswith("k_rpass (split: k_rpass<")
            assert k["scale"].startswith("k_rscale")
        if l <= 256:
            assert k["scale"].startswith("(fused into the last inverse column pass)")
        assert k["combine"] == "k_combine1 + k_cwrap + k_cfix (cyclic)"
        pw = k["pointwise"]
        if kind == SQR:
            assert pw.startswith("k_pwsq") or pw.endswith("(B = A)")
        elif kind == PRE:
            assert pw.startswith("k_pwsp") or pw.endswith("(B cached)")
        else:
            assert not pw.endswith(("(B = A)", "(B cached)")) and not pw.startswith(("k_pwsq", "k_pwsp")), pw


def test_version_has_the_mulmodm1_entries(mp):
    assert mp.lib().mpfft_version() >= 6
    for name in ("mpfft_mulmodm1_check_params", "mpfft_mulmodm1_ex", "mpfft_sqrmodm1_ex", "mpfft_mulmodm1_device",
                 "mpfft_sqrmodm1_device", "mpfft_mulmodm1_workspace_bytes", "mpfft_mulmodm1_plan_info",
                 "mpfft_mulmodm1_workspace_layout", "mpfft_mulmodm1_stage", "mpfft_mulmodm1_stage_kernels",
                 "mpfft_mulmodm1_choose", "mpfft_mulmodm1_next_size", "mpfft_mulmodm1_precomp_bytes",
                 "mpfft_mulmodm1_precomp_device", "mpfft_mulmodm1_mul_precomp_device"):
        assert hasattr(mp.lib(), name), name


def test_every_existing_mulmod_answer_is_unchanged(mp):
    """the mod 2^B + 1 entries against the answers recorded before the cyclic entries existed"""
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
