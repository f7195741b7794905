"""CPU-only checks of the small matrix products (mpfft_matmul_*, include/mpfft.h): no device is touched.

- status codes for every m, k, p outside [1, 4], and for null pointers and a short workspace
- validity equal to dot_check_params(k, ...) over a grid
- the workspace: the dot workspace at the front, m k + k p disjoint caches at 256-byte offsets behind it,
  its size growing with m, k and p
- the kernel-name strings per pointwise family
- the inner ring's headroom for a sum of four products, restated in integers
- the version
"""
import ctypes
import itertools

import pytest

EINVAL, ETOOBIG, EUNSUPPORTED, ENOMEM = 1, 2, 3, 4
DIMS = (1, 2, 3, 4)
BAD = (0, 5, -1, 64)


def _mm():
    """the bindings of this family: the submodule mpir_fft_amd.matmul (the package is loaded by the mp fixture)"""
    import mpir_fft_amd.matmul
    return mpir_fft_amd.matmul


def test_version_has_the_matmul_entries(mp):
    assert mp.lib().mpfft_version() >= 10
    assert _mm().MM_MAX == 4
    assert (_mm().STAGE_MM_STORE, _mm().STAGE_MM_POINTWISE) == (12, 13)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("bad", BAD)
def test_a_dimension_outside_the_range_is_einval(mp, which, bad):
    lib = mp.lib()
    dims = [2, 2, 2]
    dims[which] = bad
    out = (ctypes.c_size_t * 14)()
    buf = ctypes.create_string_buffer(768)
    e = (ctypes.c_int * 4)()
    assert _mm().matmul_check_params(*dims, 100, 100, 9, 2) == EINVAL
    assert _mm().matmul_workspace_bytes(*dims, 100, 100, 9, 2) == 0
    assert lib.mpfft_matmul_workspace_layout(*dims, 100, 100, 9, 2, out) == EINVAL
    assert lib.mpfft_matmul_stage_kernels(*dims, 100, 100, 9, 2, buf, len(buf)) == EINVAL
    assert lib.mpfft_matmul_device(None, *dims, None, None, 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_matmul_ex(None, *dims, None, None, 100, 100, 9, 2) == EINVAL
    assert lib.mpfft_matmul_auto(None, *dims, None, None, 100, 100) == EINVAL
    for st in (_mm().STAGE_MM_STORE, _mm().STAGE_MM_POINTWISE, mp.STAGE_POINTWISE):
        assert lib.mpfft_matmul_stage(st, *dims, None, None, None, 100, 100, 9, 2, None, 0, None, 1, e, e) == EINVAL
    with pytest.raises(mp.MpfftError):
        _mm().matmul_workspace_layout(*dims, 100, 100, 9, 2)


def test_null_pointers_and_a_short_workspace(mp):
    lib = mp.lib()
    e = (ctypes.c_int * 4)()
    four = (ctypes.c_void_p * 4)(8, 8, 8, 8)   # non-null entries: never dereferenced before the workspace check
    assert lib.mpfft_matmul_device(None, 2, 2, 2, four, four, 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_matmul_device(four, 2, 2, 2, None, four, 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_matmul_device(four, 2, 2, 2, four, (ctypes.c_void_p * 4)(8, 8, 0, 8), 100, 100, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_matmul_device(four, 2, 2, 2, four, four, 100, 100, 9, 2, None, 0, None) == ENOMEM
    assert lib.mpfft_matmul_ex(None, 2, 2, 2, four, four, 100, 100, 9, 2) == EINVAL
    # the two stages of this family: a workspace, then their entry lists
    assert lib.mpfft_matmul_stage(_mm().STAGE_MM_STORE, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 1, e, e) == ENOMEM
    assert lib.mpfft_matmul_stage(_mm().STAGE_MM_POINTWISE, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 2, e, e) == ENOMEM
    assert lib.mpfft_matmul_stage(_mm().STAGE_MM_POINTWISE, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 2, None, e) == EINVAL
    assert lib.mpfft_matmul_stage(_mm().STAGE_MM_STORE | mp.STAGE_ACC, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 1, e, e) == EINVAL
    # every other stage is the dot's, with its codes
    assert lib.mpfft_matmul_stage(mp.STAGE_POINTWISE, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 0, None, None) == ENOMEM
    assert lib.mpfft_matmul_stage(mp.STAGE_SCALE | mp.STAGE_ACC, 2, 2, 2, None, None, None, 100, 100, 9, 2, None, 0, None, 0, None, None) == EINVAL


GRID = [(9, 2, 120, 97), (9, 2, 0, 5), (4, 3, 5, 5), (1, 64, 5, 5), (13, 64, 100, 100), (11, 8, 5000, 4000),
        (8, 512, 140000, 140000), (8, 512, 300000, 300000), (7, 1024, 131064, 100), (6, 4096, 131000, 131000),
        (15, 4, 20000000, 20000000), (6, 1024, 32760, 32760)]


@pytest.mark.parametrize("depth,w,n1,n2", GRID)
def test_validity_is_the_dots_at_k(mp, depth, w, n1, n2):
    seen = set()
    for m, k, p in itertools.product(DIMS, repeat=3):
        want = mp.dot_check_params(k, n1, n2, depth, w)
        assert _mm().matmul_check_params(m, k, p, n1, n2, depth, w) == want, (m, k, p)
        assert (_mm().matmul_workspace_bytes(m, k, p, n1, n2, depth, w) > 0) == (want == 0)
        seen.add(want)
    assert len(seen) == 1 or ETOOBIG in seen   # the dot bound tightens with k only
    for k in DIMS:   # just above the dot's operand bound
        n = mp.dot_max_limbs(k, depth, w) if depth >= 2 and ((1 << depth) * w) % 64 == 0 and (1 << depth) * w // 64 <= 4096 else None
        if n:
            assert _mm().matmul_check_params(2, k, 2, n, n, depth, w) == 0
            assert _mm().matmul_check_params(2, k, 2, n + 1, n + 1, depth, w) == ETOOBIG


@pytest.mark.parametrize("depth,w,n1,n2", [(15, 4, 20000000, 20000000), (7, 1024, 131000, 90000), (8, 512, 140000, 140000),
                                            (6, 4096, 100000, 100000), (11, 8, 5000, 4000), (9, 2, 120, 97)])
def test_workspace_layout(mp, depth, w, n1, n2):
    for m, k, p in [(1, 1, 1), (2, 2, 2), (2, 2, 1), (1, 2, 2), (2, 3, 4), (4, 1, 2), (3, 3, 3), (4, 4, 4)]:
        lay = _mm().matmul_workspace_layout(m, k, p, n1, n2, depth, w)
        dot = mp.dot_workspace_layout(k, n1, n2, depth, w)
        total = _mm().matmul_workspace_bytes(m, k, p, n1, n2, depth, w)
        assert {x: lay[x] for x in dot} == dot   # the dot workspace at the front
        assert lay["ncache"] == m * k + k * p
        assert lay["cache0"] % 256 == 0 and lay["stride"] % 256 == 0
        assert lay["cache0"] >= mp.dot_workspace_bytes(k, n1, n2, depth, w)
        # a cache holds what mpfft_precomp_* stores for the dot plan's live slots
        P = mp.dot_plan_info(k, n1, n2, depth, w)
        assert lay["stride"] >= P["trunc"] * P["l"] * 8
        spans = [(lay["cache0"] + e * lay["stride"], lay["stride"]) for e in range(lay["ncache"])]
        for (o0, s0), (o1, _) in zip(spans, spans[1:]):
            assert o0 + s0 <= o1 and o1 % 256 == 0
        assert spans[-1][0] + spans[-1][1] == total


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (11, 8, 5000), (9, 2, 120)])
def test_workspace_grows_with_every_dimension(mp, depth, w, n):
    nb = lambda m, k, p: _mm().matmul_workspace_bytes(m, k, p, n, n, depth, w)
    for m, k, p in itertools.product((1, 2, 3), repeat=3):
        assert nb(m + 1, k, p) > nb(m, k, p)
        assert nb(m, k, p + 1) > nb(m, k, p)
        assert nb(m, k + 1, p) > nb(m, k, p)
        # a cache per matrix entry, nothing per result entry
        stride = _mm().matmul_workspace_layout(m, k, p, n, n, depth, w)["stride"]
        assert nb(m + 1, k, p) - nb(m, k, p) == k * stride
        assert nb(m, k, p + 1) - nb(m, k, p) == k * stride
    # the size is a function of the shape alone
    assert nb(2, 2, 2) == nb(2, 2, 2)


@pytest.mark.parametrize("m,k,p,depth,w,n,store,mm", [
    (2, 2, 2, 15, 4, 20000000, "k_pwsx<18> quad + last two row levels", "k_pwmm<18>"),
    (2, 4, 1, 6, 4096, 131000, "k_pwsx<20> pair + last row level", "k_pwmm<20>"),
    (3, 3, 3, 7, 1024, 131000, "k_pwsx<18> (nested", "k_pwmm<18>"),
    (2, 2, 2, 11, 8, 5000, "k_pwm2", "k_slotacc"), (2, 2, 1, 9, 16, 1000, "k_pwm ", "k_slotacc"),
    (4, 4, 4, 8, 8, 100, "k_pw ", "k_slotacc"), (1, 2, 2, 9, 2, 120, "k_pointwise", "k_slotacc")])
def test_matmul_stage_kernels(mp, m, k, p, depth, w, n, store, mm):
    sk = _mm().matmul_stage_kernels(m, k, p, n, n, depth, w)
    dot = mp.dot_stage_kernels(k, n, n, depth, w)
    assert set(sk) == set(mp.STAGE_NAMES)
    for f in mp.STAGE_NAMES:
        if f != "pointwise":
            assert sk[f] == dot[f], f
    first, later = sk["pointwise"].split(" + k_")
    later = "k_" + later
    assert first.startswith(store), sk["pointwise"]
    assert later.startswith(mm), sk["pointwise"]
    if mm.startswith("k_pwmm"):
        assert "single launch" in later, sk["pointwise"]
        # the caches are written with the loaders of the dot's first-term kernel
        assert first == dot["pointwise"].split(" + k_")[0].replace("k_pwss", "k_pwsx")
    else:
        assert first.endswith("(B cached)"), sk["pointwise"]


def test_nested_names_under_the_pointwise_selector(mp, monkeypatch):
    monkeypatch.setenv("MPFFT_POINTWISE", "pwss")
    sk = _mm().matmul_stage_kernels(2, 2, 2, 32000, 32000, 6, 1024)
    assert sk["pointwise"].startswith("k_pwsx<10> (nested") and " + k_pwmm<10> (" in sk["pointwise"]


@pytest.mark.parametrize("M,K,l", [(10, 256, 1024), (18, 256, 2048), (20, 512, 4096)])
def test_inner_headroom_for_four_products(M, K, l):
    """A slot is cut into K pieces of B = 64 l / K bits; behind the quad loaders a piece is below 2^(B + 2)
    in magnitude, so a coefficient of one slot's negacyclic convolution is below K 2^(2 B + 4) and a sum of
    MM_MAX = 4 of them below K 2^(2 B + 6).  It is read off its residue mod 2^N' + 1, N' = 64 M, as a signed
    number, which needs it below 2^(N' - 1): N' >= 2 B + lk + 4 + 2 + 2."""
    B, lk = 64 * l // K, K.bit_length() - 1
    assert 1 << lk == K and B * K == 64 * l
    piece = 1 << (B + 2)
    coeff = K * piece * piece          # one product's bound
    assert 4 * coeff <= 1 << (64 * M - 1)
    assert 64 * M >= 2 * B + lk + 4 + 2
    assert 64 * M >= 2 * B + lk + 6 + 2   # with the quad loaders' two bits
    # the pending exponents of two records add up below the meta word's 12 bits twice over
    assert 2 * 64 * M <= 4096
    # the issue's figures: 524, 1036 and 1037 bits needed for one product, at least 116 spare
    assert 64 * M - (2 * B + lk + 4) >= 116
