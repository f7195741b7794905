"""CPU-only checks of the signed sums of products (mpfft_sdot_*, include/mpfft.h): no device is touched.

- the version, validation and status codes (a mask bit at or above K, K outside [1, 64], the dot's codes)
- the workspace: the dot's layout, then the complement scratch and D, disjoint, aligned, independent of neg
- sdot_stage_kernels against dot_stage_kernels
- the identity the feature rests on, restated in Python integers
- the mask and the two's-complement helpers of the Python layer
"""
import ctypes
import random

import numpy as np
import pytest

from test_dot_cpu import SHAPES

EINVAL, ETOOBIG, EUNSUPPORTED, ENOMEM = 1, 2, 3, 4
KS = (1, 2, 3, 4, 64)
SDNEG = "k_sdneg + "
SDFIX = " + k_sdedge + k_sdfix (blocks of 4096 limbs)"


def test_version_has_the_sdot_entries(mp):
    assert mp.lib().mpfft_version() >= 9
    assert (mp.STAGE_SD_NEG, mp.STAGE_SD_FIX) == (10, 11)
    assert mp.SDOT_FIX_BLOCK == 4096


def _every_entry_with_neg(mp, K, neg, n1=100, n2=100, depth=9, w=2):
    """the status of every entry that takes the mask, for null pointers"""
    lib = mp.lib()
    buf = ctypes.create_string_buffer(768)
    return [lib.mpfft_sdot_check_params(K, neg, n1, n2, depth, w),
            lib.mpfft_sdot_device(None, K, neg, None, None, n1, n2, depth, w, None, 0, None),
            lib.mpfft_sdot_ex(None, K, neg, None, None, n1, n2, depth, w),
            lib.mpfft_sdot_auto(None, K, neg, None, None, n1, n2),
            lib.mpfft_sdot_stage_kernels(K, neg, n1, n2, depth, w, buf, len(buf))]


@pytest.mark.parametrize("K,neg", [(1, 2), (1, 3), (2, 4), (2, 7), (3, 1 << 3), (4, 1 << 63), (63, 1 << 63), (5, (1 << 64) - 1)])
def test_a_mask_bit_at_or_above_k_is_einval(mp, K, neg):
    assert _every_entry_with_neg(mp, K, neg) == [EINVAL] * 5
    assert mp.dot_check_params(K, 100, 100, 9, 2) == 0


@pytest.mark.parametrize("K,neg", [(1, 1), (2, 3), (3, 5), (64, (1 << 64) - 1), (64, 1 << 63), (7, 0)])
def test_a_mask_inside_k_is_accepted(mp, K, neg):
    st = _every_entry_with_neg(mp, K, neg)
    assert st[0] == 0 and st[4] == 0
    assert st[1] == EINVAL and st[2] == EINVAL and st[3] == EINVAL   # the null pointers, behind the parameter checks


@pytest.mark.parametrize("K", [0, 65, -1, 1000])
def test_k_outside_the_range_is_einval(mp, K):
    lib = mp.lib()
    out = (ctypes.c_size_t * 13)()
    assert _every_entry_with_neg(mp, K, 0) == [EINVAL] * 5
    assert _every_entry_with_neg(mp, K, 1) == [EINVAL] * 5
    assert lib.mpfft_sdot_workspace_layout(K, 100, 100, 9, 2, out) == EINVAL
    assert lib.mpfft_sdot_workspace_bytes(K, 100, 100, 9, 2) == 0
    for st in (mp.STAGE_SD_NEG, mp.STAGE_SD_FIX, mp.STAGE_POINTWISE):
        assert lib.mpfft_sdot_stage(st, K, None, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL


@pytest.mark.parametrize("depth,w", SHAPES)
def test_the_other_codes_are_the_dots(mp, depth, w):
    for K in KS:
        n = mp.dot_max_limbs(K, depth, w)
        for n1, n2 in ((n, n), (n + 1, n + 1), (0, 5), (5, 0), (1, 1), (n, 1)):
            want = mp.dot_check_params(K, n1, n2, depth, w)
            for neg in (0, 1, 1 << (K - 1), (1 << K) - 1):
                assert mp.sdot_check_params(K, neg, n1, n2, depth, w) == want, (K, neg, n1, n2)
            assert (mp.sdot_workspace_bytes(K, n1, n2, depth, w) == 0) == (want != 0)
        assert mp.sdot_check_params(K, 0, n + 1, n + 1, depth, w) == ETOOBIG


def test_codes_of_invalid_shapes_and_stages(mp):
    lib = mp.lib()
    for n1, n2, depth, w, code in ((0, 5, 9, 2, EINVAL), (5, 5, 4, 3, EINVAL), (5, 5, 1, 64, EINVAL), (100, 100, 13, 64, EUNSUPPORTED)):
        for K in KS:
            assert mp.dot_check_params(K, n1, n2, depth, w) == code
            assert mp.sdot_check_params(K, 1, n1, n2, depth, w) == code
    # a workspace that is too small, for the new stages and the forwarded ones
    for st in (mp.STAGE_SD_NEG, mp.STAGE_SD_NEG | mp.STAGE_ACC, mp.STAGE_SD_FIX, mp.STAGE_POINTWISE, mp.STAGE_POINTWISE | mp.STAGE_ACC):
        assert lib.mpfft_sdot_stage(st, 2, None, None, None, 100, 100, 9, 2, None, 0, None) == ENOMEM
    assert lib.mpfft_sdot_device(None, 2, 1, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL
    # the accumulate flag belongs to the pointwise stage and the pre-pass
    for st in (mp.STAGE_FWD_COLUMNS, mp.STAGE_FWD_ROWS, mp.STAGE_INV_ROWS, mp.STAGE_INV_COLUMNS, mp.STAGE_SCALE, mp.STAGE_COMBINE,
               mp.STAGE_SD_FIX):
        assert lib.mpfft_sdot_stage(st | mp.STAGE_ACC, 2, None, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL
    # the dot's stage entry does not know the new stages
    for st in (mp.STAGE_SD_NEG, mp.STAGE_SD_FIX):
        assert lib.mpfft_dot_stage(st, 2, None, None, None, 100, 100, 9, 2, ctypes.c_void_p(256), 1 << 40, None) == EINVAL


@pytest.mark.parametrize("depth,w,n1,n2", [(15, 4, 20000000, 20000000), (7, 1024, 131000, 131000), (8, 512, 220000, 60000),
                                            (8, 512, 60000, 220000), (11, 8, 5000, 300), (9, 2, 120, 97), (9, 2, 1, 1)])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_workspace_layout(mp, depth, w, n1, n2, K):
    lay = mp.sdot_workspace_layout(K, n1, n2, depth, w)
    dot = mp.dot_workspace_layout(K, n1, n2, depth, w)
    assert list(lay.values())[:11] == list(dot.values())
    total = mp.sdot_workspace_bytes(K, n1, n2, depth, w)
    dot_total = mp.dot_workspace_bytes(K, n1, n2, depth, w)
    l = mp.dot_plan_info(K, n1, n2, depth, w)["l"]
    slots, cbw = lay["slots"], lay["cbw"]
    spans = []
    for x in "ABC":
        spans += [(lay["dig" + x], slots * l * 8), (lay["top" + x], slots * 4), (lay["cb" + x], slots * cbw * 8)]
    spans += [(lay["scratch"], 8 * n1), (lay["D"], 8 * n2 + n2)]   # D: the limbs and an overflow byte per limb
    spans.sort()
    for (o0, s0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + s0 <= o1
    assert spans[-1][0] + spans[-1][1] <= total
    assert lay["scratch"] % 256 == 0 and lay["D"] % 256 == 0
    # behind the whole dot workspace (its flags and meta words too), which therefore is valid at the front
    assert dot_total <= lay["scratch"] < lay["D"] < total
    # the size follows the plan alone: there is no mask to depend on, and K moves it as it moves the dot's
    assert total - dot_total == mp.sdot_workspace_bytes(64, n1, n2, depth, w) - mp.dot_workspace_bytes(64, n1, n2, depth, w)


@pytest.mark.parametrize("K,depth,w,n", [(2, 15, 4, 20000000), (4, 6, 4096, 131000), (3, 7, 1024, 131000), (2, 11, 8, 5000),
                                         (2, 9, 16, 1000), (64, 8, 8, 100), (2, 9, 2, 120), (1, 5, 4096, 20000)])
def test_sdot_stage_kernels(mp, K, depth, w, n):
    lib = mp.lib()
    b0, b1 = ctypes.create_string_buffer(768), ctypes.create_string_buffer(768)
    assert lib.mpfft_dot_stage_kernels(K, n, n, depth, w, b0, len(b0)) == 0
    assert lib.mpfft_sdot_stage_kernels(K, 0, n, n, depth, w, b1, len(b1)) == 0
    assert b0.value == b1.value   # byte-equal
    dot = mp.dot_stage_kernels(K, n, n, depth, w)
    for neg in (1, 1 << (K - 1), (1 << K) - 1):
        sk = mp.sdot_stage_kernels(K, neg, n, n, depth, w)
        assert set(sk) == set(mp.STAGE_NAMES)
        for k in mp.STAGE_NAMES:
            if k == "fwd_columns":
                assert sk[k] == SDNEG + dot[k]
            elif k == "combine":
                assert sk[k] == dot[k] + SDFIX
            else:
                assert sk[k] == dot[k], k
    assert str(mp.SDOT_FIX_BLOCK) in SDFIX


def _pack(x, bits1, j, S):
    """the j pieces of x, bits1 bits each, S bits apart"""
    m = (1 << bits1) - 1
    assert x >> (bits1 * j) == 0 and S % 8 == 0   # j pieces hold it
    return int.from_bytes(b"".join(((x >> (i * bits1)) & m).to_bytes(S // 8, "little") for i in range(j)), "little")


@pytest.mark.parametrize("depth,w", [(9, 2), (8, 8)])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_the_identity_in_integers(mp, depth, w, K):
    """At dot_max_limbs: the complement of any a has n1 limbs and as many pieces below 2^bits1, so every
    coefficient of the summed convolutions of the fed terms stays below 2^N, and r' - X D + D is the
    signed sum mod 2^(64 (n1 + n2 + 1)).  The convolutions are formed by Kronecker substitution (pieces
    S bits apart, S past any coefficient)."""
    N = (1 << depth) * w
    n = mp.dot_max_limbs(K, depth, w)
    P = mp.dot_plan_info(K, n, n, depth, w)
    bits1, j = P["bits1"], P["j1"]
    S = N + 64
    X = 1 << (64 * n)
    M = 1 << (64 * (2 * n + 1))
    ones = X - 1
    rng = random.Random(0x5d07 + 131 * depth + K)
    pool = [rng.getrandbits(64 * n) for _ in range(min(K, 3))]   # (K = 64: three random values, repeated)
    kinds = {"ones": lambda: ones, "zero": lambda: 0, "random": lambda: rng.choice(pool)}
    full = (1 << K) - 1
    largest = 0
    cache = {}   # the Kronecker product of a fed operand and a b, each pair once
    prods = {}

    def mul(x, y):   # (operands repeat between terms and cases)
        if (x, y) not in prods:
            prods[(x, y)] = x * y
        return prods[(x, y)]
    for ka in kinds:
        for kb in kinds:
            a = [kinds[ka]() for _ in range(K)]
            b = [kinds[kb]() for _ in range(K)]
            masks = {full, rng.getrandbits(K) | 1} if K == 64 else {0, 1, full, rng.getrandbits(K)}
            for neg in sorted(masks):
                fed = [(ones - a[i]) if (neg >> i) & 1 else a[i] for i in range(K)]
                assert all(0 <= f < X for f in fed)
                conv = 0
                for f, y in zip(fed, b):
                    if (f, y) not in cache:
                        cache[(f, y)] = _pack(f, bits1, j, S) * _pack(y, bits1, j, S)
                    conv += cache[(f, y)]
                raw = conv.to_bytes(2 * j * S // 8, "little")   # (raises if a coefficient lies past 2 j)
                coef = [int.from_bytes(raw[k * S // 8:(k + 1) * S // 8], "little") for k in range(2 * j)]
                assert max(coef) < 1 << N, (ka, kb, neg)
                largest = max(largest, max(coef))
                rp = sum(c << (k * bits1) for k, c in enumerate(coef))   # what the combine forms
                assert rp == sum(mul(f, y) for f, y in zip(fed, b)) and rp < K << (128 * n)
                D = sum(b[i] for i in range(K) if (neg >> i) & 1)
                assert D < 1 << (64 * (n + 1))
                want = sum((-1 if (neg >> i) & 1 else 1) * mul(a[i], b[i]) for i in range(K))
                got = (rp - X * D + D) % M
                assert got == want % M
                lim = np.frombuffer(got.to_bytes(8 * (2 * n + 1), "little"), dtype=np.uint64)
                assert mp.sdot_to_int(lim) == want
                top = int(lim[-1])
                assert top < K or top >= (1 << 64) - K
    # (the sum of complemented zeros times all-ones reaches the dot's own worst case)
    assert largest == K * max((_pack(ones, bits1, j, S) ** 2 >> (k * S)) & ((1 << S) - 1) for k in (j - 2, j - 1, j))


def test_neg_mask_and_to_int(mp):
    assert mp._neg_mask(5) == 5 and mp._neg_mask([True, False, True]) == 5 and mp._neg_mask((0, 1)) == 2
    assert mp._neg_mask(np.uint64(1 << 63)) == 1 << 63 and mp._neg_mask([]) == 0
    with pytest.raises(ValueError):
        mp._neg_mask(1 << 64)
    with pytest.raises(ValueError):
        mp._neg_mask(-1)
    assert mp.sdot_check_params(3, [False, True, False], 100, 100, 9, 2) == 0
    assert mp.sdot_check_params(2, [False, False, True], 100, 100, 9, 2) == EINVAL
    ones = np.full(3, np.iinfo(np.uint64).max, dtype=np.uint64)
    assert mp.sdot_to_int(ones) == -1
    assert mp.sdot_to_int(np.array([5, 0], dtype=np.uint64)) == 5
    assert mp.sdot_to_int(np.array([0, 1 << 63], dtype=np.uint64)) == -(1 << 127)
    assert mp.sdot_to_int(np.array([0, (1 << 64) - 64], dtype=np.uint64)) == -64 << 64
