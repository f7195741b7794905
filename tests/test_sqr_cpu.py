"""CPU-only checks of the squaring entries (mpfft_sqr_*, include/mpfft.h): no device is touched.

- the square's workspace is the multiply's for (n, n) less operand B's three arrays
- mpfft_sqr_stage_kernels names k_pwsq on nested plans and "<kernel> (B = A)" elsewhere, and
  equals the multiply's fields everywhere else
- invalid parameters return the codes of mpfft_check_params(n, n, depth, w)
"""
import ctypes

import numpy as np
import pytest

EINVAL, ETOOBIG, EUNSUPPORTED = 1, 2, 3


def _align256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("depth,w,n", [(15, 4, 20312500), (7, 1024, 131064), (11, 8, 5000), (9, 2, 120)])
def test_sqr_workspace_is_the_multiplys_less_operand_b(mp, depth, w, n):
    lay = mp.workspace_layout(n, n, depth, w)
    l = mp.plan_info(n, n, depth, w)["l"]
    slots, cbw = lay["slots"], lay["cbw"]
    assert slots == 2 << depth
    b_bytes = slots * l * 8 + _align256(slots * 4) + _align256(slots * cbw * 8)
    assert mp.sqr_workspace_bytes(n, depth, w) == mp.workspace_bytes(n, n, depth, w) - b_bytes
    sl = mp.sqr_workspace_layout(n, depth, w)
    assert (sl["digA"], sl["topA"], sl["cbA"]) == (lay["digA"], lay["topA"], lay["cbA"])
    assert (sl["digB"], sl["topB"], sl["cbB"]) == (0, 0, 0)
    assert (sl["slots"], sl["cbw"]) == (slots, cbw)


@pytest.mark.parametrize("depth,w,n,head,tail", [
    (15, 4, 20312500, "k_pwsq<18>", "quad + last two row levels"),
    (6, 4096, 131064, "k_pwsq<20>", "pair + last row level"),
    (11, 8, 5000, None, "(B = A)")])
def test_sqr_stage_kernels(mp, depth, w, n, head, tail):
    sq = mp.sqr_stage_kernels(n, depth, w)
    mu = mp.stage_kernels(n, n, depth, w)
    pw = sq["pointwise"]
    if head:
        assert pw.startswith(head), pw
        assert mu["pointwise"].startswith(head.replace("k_pwsq", "k_pwss")), mu["pointwise"]
        assert pw == mu["pointwise"].replace("k_pwss", "k_pwsq")   # the same pair / quad suffix
    else:
        assert pw == mu["pointwise"] + " (B = A)" and not pw.startswith("k_pws"), pw
    assert tail in pw, pw
    for k in mp.STAGE_NAMES:
        if k != "pointwise":
            assert sq[k] == mu[k], k


def test_sqr_parameter_errors(mp):
    lib = mp.lib()
    r = np.zeros(8, np.uint64)
    a = np.ones(4, np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    out = (ctypes.c_size_t * 8)()
    buf = ctypes.create_string_buffer(512)
    # (n, depth, w): n = 0; a square that does not fit the convolution; coefficients of 8192 limbs
    for n, depth, w, code in ((0, 9, 2, EINVAL), (100000, 6, 1, ETOOBIG), (100, 13, 64, EUNSUPPORTED)):
        assert mp.check_params(max(n, 0), max(n, 0), depth, w) == code
        assert lib.mpfft_sqr_workspace_layout(n, depth, w, out) == code
        assert lib.mpfft_sqr_stage_kernels(n, depth, w, buf, len(buf)) == code
        assert lib.mpfft_sqr_workspace_bytes(n, depth, w) == 0
        assert lib.mpfft_sqr_device(None, None, n, depth, w, None, 0, None) == code
        assert lib.mpfft_sqr_stage(mp.STAGE_POINTWISE, None, None, n, depth, w, None, 0, None) == code
        assert lib.mpfft_sqr_ex(p(r), p(a), n, depth, w) == code
    with pytest.raises(mp.MpfftError):
        mp.sqr_stage_kernels(0, 9, 2)


def test_version_has_the_squaring_entries(mp):
    assert mp.lib().mpfft_version() >= 3
