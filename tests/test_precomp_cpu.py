"""CPU-only checks of the precomputed-operand entries (mpfft_precomp_*, mpfft_mul_precomp_*,
include/mpfft.h): no device is touched.

- the cache is one record of K (8 M + 4) bytes per live slot on nested plans, and the live slots
  of operand B's limb and carry-limb arrays on the others
- the multiply against it needs the multiply's workspace less operand B's three arrays
- mpfft_precomp_stage_kernels names k_pwsx / k_pwsp on nested plans and "copy" / "<kernel> (B cached)"
  elsewhere, and equals the multiply's fields everywhere else
- invalid parameters return the codes of mpfft_check_params(n1, n2, depth, w)
"""
import ctypes
import os

import numpy as np
import pytest

EINVAL, ETOOBIG, EUNSUPPORTED, ENOMEM = 1, 2, 3, 4


def _align256(x):
    return (x + 255) // 256 * 256


class _pointwise_env:
    def __init__(self, kind):
        self.kind = kind

    def __enter__(self):
        self.old = os.environ.get("MPFFT_POINTWISE")
        if self.kind is None:
            os.environ.pop("MPFFT_POINTWISE", None)
        else:
            os.environ["MPFFT_POINTWISE"] = self.kind

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("MPFFT_POINTWISE", None)
        else:
            os.environ["MPFFT_POINTWISE"] = self.old


# (depth, w, n1, n2, MPFFT_POINTWISE, K, M): C3, l = 4096, unbalanced l = 2048, l = 1024 under pwss
@pytest.mark.parametrize("depth,w,n1,n2,kind,K,M", [
    (15, 4, 20312500, 20312500, None, 256, 18),
    (6, 4096, 131064, 131064, None, 512, 20),
    (8, 512, 200000, 60000, None, 256, 18),
    (6, 1024, 32760, 32760, "pwss", 256, 10)])
def test_cache_is_one_record_per_live_slot_on_nested_plans(mp, depth, w, n1, n2, kind, K, M):
    with _pointwise_env(kind):
        P = mp.plan_info(n1, n2, depth, w)
        assert mp.precomp_stage_kernels(n1, n2, depth, w)["precomp"].startswith("k_pwsx<%d>" % M)
        assert 64 * P["l"] // K * 2 + (K.bit_length() - 1) + 4 <= 64 * M   # the inner ring holds the pieces
        assert mp.precomp_bytes(n1, n2, depth, w) == P["trunc"] * K * (8 * M + 4)
    if depth == 15:
        assert 1.5e9 < P["trunc"] * K * (8 * M + 4) < 1.53e9   # C3: about 1.5 GB


@pytest.mark.parametrize("depth,w,n1,n2", [(11, 8, 5000, 5000), (9, 2, 120, 97), (9, 16, 4000, 3000), (11, 8, 261952, 261952)])
def test_cache_is_b_row_arrays_on_the_other_families(mp, depth, w, n1, n2):
    P = mp.plan_info(n1, n2, depth, w)
    assert mp.precomp_stage_kernels(n1, n2, depth, w)["precomp"] == "copy"
    # the live slots of B's limbs and of its carry limbs (canonical: no carry masks)
    assert mp.precomp_bytes(n1, n2, depth, w) == P["trunc"] * P["l"] * 8 + _align256(P["trunc"] * 4)


@pytest.mark.parametrize("depth,w,n1,n2", [(15, 4, 20312500, 20312500), (7, 1024, 131064, 131064), (8, 512, 60000, 200000),
                                           (11, 8, 5000, 5000), (9, 2, 120, 97)])
def test_workspace_is_the_multiplys_less_operand_b(mp, depth, w, n1, n2):
    lay = mp.workspace_layout(n1, n2, depth, w)
    l = mp.plan_info(n1, n2, depth, w)["l"]
    slots, cbw = lay["slots"], lay["cbw"]
    b_bytes = slots * l * 8 + _align256(slots * 4) + _align256(slots * cbw * 8)
    assert mp.mul_precomp_workspace_bytes(n1, n2, depth, w) == mp.workspace_bytes(n1, n2, depth, w) - b_bytes
    if n1 == n2:
        assert mp.mul_precomp_workspace_bytes(n1, n2, depth, w) == mp.sqr_workspace_bytes(n1, depth, w)


@pytest.mark.parametrize("depth,w,n1,n2,head,tail", [
    (15, 4, 20312500, 20312500, "k_pwss<18>", "quad + last two row levels"),
    (6, 4096, 131064, 131064, "k_pwss<20>", "pair + last row level"),
    (7, 1024, 131064, 131064, "k_pwss<18>", ""),
    (11, 8, 5000, 5000, None, "(B cached)"),
    (9, 2, 120, 97, None, "(B cached)")])
def test_precomp_stage_kernels(mp, depth, w, n1, n2, head, tail):
    pk = mp.precomp_stage_kernels(n1, n2, depth, w)
    mu = mp.stage_kernels(n1, n2, depth, w)
    assert list(pk) == ["precomp"] + list(mp.STAGE_NAMES)
    pw = pk["pointwise"]
    if head:
        assert mu["pointwise"].startswith(head), mu["pointwise"]
        assert pw == mu["pointwise"].replace("k_pwss", "k_pwsp")            # the same pair / quad suffix
        assert pk["precomp"] == mu["pointwise"].replace("k_pwss", "k_pwsx")
    else:
        assert pw == mu["pointwise"] + " (B cached)" and not pw.startswith("k_pws"), pw
        assert pk["precomp"] == "copy"
    assert tail in pw, pw
    for k in mp.STAGE_NAMES:
        if k != "pointwise":
            assert pk[k] == mu[k], k


def test_parameter_errors(mp):
    lib = mp.lib()
    r = np.zeros(8, np.uint64)
    a = np.ones(4, np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    buf = ctypes.create_string_buffer(640)
    h = ctypes.c_void_p()
    # (n1, n2, depth, w): n2 = 0; n1 = 0; a product that does not fit; coefficients of 8192 limbs; n w not whole limbs
    for n1, n2, depth, w, code in ((4, 0, 9, 2, EINVAL), (0, 4, 9, 2, EINVAL), (100000, 100000, 6, 1, ETOOBIG),
                                   (100, 100, 13, 64, EUNSUPPORTED), (4, 4, 5, 3, EINVAL)):
        assert mp.check_params(n1, n2, depth, w) == code
        assert lib.mpfft_precomp_bytes(n1, n2, depth, w) == 0
        assert lib.mpfft_mul_precomp_workspace_bytes(n1, n2, depth, w) == 0
        assert lib.mpfft_precomp_stage_kernels(n1, n2, depth, w, buf, len(buf)) == code
        assert lib.mpfft_precomp_device(None, 0, None, n1, n2, depth, w, None, 0, None) == code
        assert lib.mpfft_mul_precomp_device(None, None, n1, None, 0, n2, depth, w, None, 0, None) == code
        for st in (mp.STAGE_FWD_COLUMNS, mp.STAGE_PRE_STORE):
            assert lib.mpfft_precomp_stage(st, None, 0, None, n1, n2, depth, w, None, 0, None) == code
        assert lib.mpfft_mul_precomp_stage(mp.STAGE_POINTWISE, None, None, 0, None, n1, n2, depth, w, None, 0, None) == code
        assert lib.mpfft_precomp_create(ctypes.byref(h), p(a), n2, n1, depth, w) == code and not h.value
    # valid parameters, no buffers: ENOMEM before anything is launched
    assert lib.mpfft_precomp_device(None, 0, None, 120, 97, 9, 2, None, 0, None) == ENOMEM
    assert lib.mpfft_mul_precomp_device(None, None, 120, None, 0, 97, 9, 2, None, 0, None) == ENOMEM
    assert lib.mpfft_precomp_stage(mp.STAGE_PRE_STORE, None, 0, None, 120, 97, 9, 2, None, 0, None) == ENOMEM
    assert lib.mpfft_precomp_stage(mp.STAGE_POINTWISE, None, 0, None, 120, 97, 9, 2, None, 0, None) == EINVAL
    assert lib.mpfft_mul_precomp_ex(p(r), p(a), 4, None) == EINVAL
    assert lib.mpfft_precomp_create(None, p(a), 4, 4, 9, 2) == EINVAL
    lib.mpfft_precomp_destroy(None)
    with pytest.raises(mp.MpfftError):
        mp.precomp_stage_kernels(0, 4, 9, 2)
    for f in (mp.alloc_precomp, mp.alloc_workspace_mul_precomp):
        with pytest.raises(mp.MpfftError) as e:
            f(0, 4, 9, 2)
        assert e.value.code == EINVAL


def test_version_has_the_precomp_entries(mp):
    assert mp.lib().mpfft_version() >= 5
