"""CPU-only checks of the sums of products (mpfft_dot_*, include/mpfft.h): no device is touched.

- validation and status codes (K outside [1, 64], ETOOBIG just above dot_max_limbs)
- the plan: bits1 = (N - depth - ceil(log2 K)) / 2, K = 1 is the multiply's plan
- the bound the feature rests on, restated in Python integers
- the workspace: three disjoint coefficient arrays inside dot_workspace_bytes
- dot_choose, dot_stage_kernels, the version
"""
import ctypes

import pytest

from helpers import max_limbs

EINVAL, ETOOBIG, EUNSUPPORTED, ENOMEM = 1, 2, 3, 4
KS = (1, 2, 3, 4, 64)
SHAPES = [(15, 4), (7, 1024), (6, 4096), (11, 8), (9, 2), (8, 8), (9, 16), (10, 2)]


def _s(K):
    return (K - 1).bit_length()   # ceil(log2 K)


def test_version_has_the_dot_entries(mp):
    assert mp.lib().mpfft_version() >= 8
    assert mp.DOT_MAX == 64


@pytest.mark.parametrize("K", [0, 65, -1, 1000])
def test_k_outside_the_range_is_einval(mp, K):
    lib = mp.lib()
    out = (ctypes.c_size_t * 11)()
    info = (ctypes.c_long * 10)()
    buf = ctypes.create_string_buffer(640)
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    assert mp.dot_check_params(K, 100, 100, 9, 2) == EINVAL
    assert lib.mpfft_dot_plan_info(K, 100, 100, 9, 2, info) == EINVAL
    assert lib.mpfft_dot_workspace_layout(K, 100, 100, 9, 2, out) == EINVAL
    assert lib.mpfft_dot_workspace_bytes(K, 100, 100, 9, 2) == 0
    assert lib.mpfft_dot_stage_kernels(K, 100, 100, 9, 2, buf, len(buf)) == EINVAL
    assert lib.mpfft_dot_choose(K, 100, 100, ctypes.byref(d), ctypes.byref(w)) == EINVAL
    assert lib.mpfft_dot_device(None, K, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_dot_stage(mp.STAGE_POINTWISE, K, None, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_dot_ex(None, K, None, None, 100, 100, 9, 2) == EINVAL


def test_the_other_codes_are_check_params(mp):
    # n = 0; N not a whole number of limbs; depth out of range; coefficients of 8192 limbs
    for n1, n2, depth, w, code in ((0, 5, 9, 2, EINVAL), (5, 5, 4, 3, EINVAL), (5, 5, 1, 64, EINVAL), (100, 100, 13, 64, EUNSUPPORTED)):
        assert mp.check_params(n1, n2, depth, w) == code
        for K in KS:
            assert mp.dot_check_params(K, n1, n2, depth, w) == code, (K, n1, n2, depth, w)
    with pytest.raises(mp.MpfftError):
        mp.dot_plan_info(2, 0, 5, 9, 2)
    # a workspace too small for a valid shape
    assert mp.lib().mpfft_dot_stage(mp.STAGE_POINTWISE, 2, None, None, None, 100, 100, 9, 2, None, 0, None) == ENOMEM
    # the accumulate flag belongs to the pointwise stage alone
    for st in (mp.STAGE_FWD_COLUMNS, mp.STAGE_FWD_ROWS, mp.STAGE_INV_ROWS, mp.STAGE_INV_COLUMNS, mp.STAGE_SCALE, mp.STAGE_COMBINE):
        assert mp.lib().mpfft_dot_stage(st | mp.STAGE_ACC, 2, None, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL


@pytest.mark.parametrize("depth,w", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_bits1_and_the_size_limit(mp, depth, w, K):
    N = (1 << depth) * w
    n = mp.dot_max_limbs(K, depth, w)
    P = mp.dot_plan_info(K, n, n, depth, w)
    assert P["bits1"] == (N - depth - _s(K)) // 2
    assert P["j1"] == P["j2"] == (64 * n - 1) // P["bits1"] + 1
    assert P["j1"] + P["j2"] - 1 <= 2 << depth
    assert P["trunc"] % (2 * P["NC"]) == 0 and P["trunc"] >= P["j1"] + P["j2"] - 1
    assert mp.dot_check_params(K, n, n, depth, w) == 0
    assert mp.dot_check_params(K, n + 1, n + 1, depth, w) == ETOOBIG
    assert n <= max_limbs(depth, w)


@pytest.mark.parametrize("depth,w,n1,n2", [(15, 4, 20312500, 20312500), (7, 1024, 131064, 100), (11, 8, 5000, 4000),
                                            (9, 2, 120, 97), (8, 512, 140000, 140000)])
def test_k1_plan_is_the_multiplys(mp, depth, w, n1, n2):
    assert mp.dot_plan_info(1, n1, n2, depth, w) == mp.plan_info(n1, n2, depth, w)
    d, m = mp.dot_stage_kernels(1, n1, n2, depth, w), mp.stage_kernels(n1, n2, depth, w)
    for k in mp.STAGE_NAMES:
        if k != "pointwise":
            assert d[k] == m[k], k
    assert d["pointwise"].startswith(m["pointwise"] + " + ")


@pytest.mark.parametrize("depth,w", [(8, 8), (9, 2), (10, 2), (6, 1024)])
def test_the_bound_in_integers(mp, depth, w):
    """All-ones operands at dot_max_limbs: every piece but the last is 2^bits1 - 1, so the largest
    coefficient of the summed convolutions is K times the middle coefficient of one product.  It is
    below 2^N under the dot's bits1 -- and for K = 2 at least 2^N + 1 under the multiply's bits1
    where N - depth is even, so the residue mod 2^N + 1 would no longer be the coefficient."""
    N = (1 << depth) * w

    def largest(K, bits1, n):
        x = (1 << (64 * n)) - 1
        j = (64 * n - 1) // bits1 + 1
        pc = [(x >> (i * bits1)) & ((1 << bits1) - 1) for i in range(j)]
        return K * max(sum(pc[i] * pc[k - i] for i in range(max(0, k - j + 1), min(k, j - 1) + 1)) for k in (j - 2, j - 1, j))
    for K in KS:
        n = mp.dot_max_limbs(K, depth, w)
        b = mp.dot_plan_info(K, n, n, depth, w)["bits1"]
        assert largest(K, b, n) < 1 << N, (K, depth, w)
    assert ((N - depth) % 2 == 0) == (depth % 2 == 0)
    if depth % 2:   # (9, 2): N - depth odd, the multiply's bits1 happens to leave one spare bit
        return
    n = max_limbs(depth, w)
    b = mp.plan_info(n, n, depth, w)["bits1"]
    assert 2 * b + depth == N
    assert largest(1, b, n) < 1 << N
    assert largest(2, b, n) >= (1 << N) + 1


def _align256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("depth,w,n", [(15, 4, 20000000), (7, 1024, 131000), (8, 512, 140000), (11, 8, 5000), (9, 2, 120)])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_workspace_holds_three_disjoint_arrays(mp, depth, w, n, K):
    lay = mp.dot_workspace_layout(K, n, n, depth, w)
    l = mp.dot_plan_info(K, n, n, depth, w)["l"]
    slots, cbw = lay["slots"], lay["cbw"]
    assert slots == 2 << depth
    total = mp.dot_workspace_bytes(K, n, n, depth, w)
    spans = []
    for x in "ABC":
        spans += [(lay["dig" + x], slots * l * 8), (lay["top" + x], slots * 4), (lay["cb" + x], slots * cbw * 8)]
    spans.sort()
    for (o0, s0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + s0 <= o1
    assert spans[-1][0] + spans[-1][1] <= total
    assert all(o % 256 == 0 for o, _ in spans)
    # the same three arrays whatever K, and one array more than a multiply that has no C
    arr = slots * l * 8 + _align256(slots * 4) + _align256(slots * cbw * 8)
    assert lay["digC"] == 2 * arr
    assert total >= 3 * arr
    assert mp.dot_workspace_bytes(64, n, n, depth, w) - total in range(0, 512)


@pytest.mark.parametrize("K,n1,n2", [(1, 1, 1), (2, 7, 3), (3, 1000, 1000), (4, 100000, 60000), (64, 3000000, 3000000),
                                     (2, 20000000, 20000000)])
def test_dot_choose_is_valid(mp, K, n1, n2):
    depth, w = mp.dot_choose(K, n1, n2)
    assert mp.dot_check_params(K, n1, n2, depth, w) == 0
    assert ((1 << depth) * w) % 64 == 0


@pytest.mark.parametrize("K,depth,w,n,head,tail", [
    (2, 15, 4, 20000000, "k_pwss<18> quad + last two row levels", "k_pwsa<18> quad + last two row levels"),
    (4, 6, 4096, 131000, "k_pwss<20> pair + last row level", "k_pwsa<20> pair + last row level"),
    (3, 7, 1024, 131000, "k_pwss<18> (nested", "k_pwsa<18> (nested"),
    (2, 11, 8, 5000, "k_pwm2", "k_slotacc"), (2, 9, 16, 1000, "k_pwm ", "k_slotacc"),
    (64, 8, 8, 100, "k_pw ", "k_slotacc"), (2, 9, 2, 120, "k_pointwise", "k_slotacc")])
def test_dot_stage_kernels(mp, K, depth, w, n, head, tail):
    sk = mp.dot_stage_kernels(K, n, n, depth, w)
    assert set(sk) == set(mp.STAGE_NAMES)
    first, later = sk["pointwise"].split(" + k_")
    assert first.startswith(head), sk["pointwise"]
    assert ("k_" + later).startswith(tail), sk["pointwise"]
    if head.startswith("k_pwss"):
        assert "k_" + later == first.replace("k_pwss", "k_pwsa")   # the same pair / quad suffix
