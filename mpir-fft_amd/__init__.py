"""mpir-fft_amd -- MI355X-native drop-in for wbhart/mpir-fft's new_mpn_mul.

Host-side mirror of the reference interface for the hot path:

    new_mpn_mul(r1, i1, n1, i2, n2, depth, w)      # /root/reference/mul_fft.c:3190

same names, same argument meaning (little-endian 64-bit limb arrays, convolution
length 2^(depth+1) over Z/(2^(2^depth * w) + 1)), computed by the hand-written
HIP kernels in csrc/ through the C ABI of libmpfft.so (include/mpfft.h).

There is no CPU fallback: if libmpfft.so is missing or no GPU is visible, every
compute entry point raises.  Errors the reference would turn into a segfault
(mul_fft.c:3186-3188) raise MpfftError with the library's reason.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPFFT_LIB=diag selects the diagnostic build libmpfft_diag.so (make DIAG=1: tuning and
# ablation knobs for scripts/; never used by the tests, smoke() or the bench)
_LIBSEL = os.environ.get("MPFFT_LIB", "")
LIB_PATH = os.path.join(_HERE, "libmpfft_diag.so" if _LIBSEL == "diag" else
                        _LIBSEL if _LIBSEL.endswith(".so") else "libmpfft.so")   # a path: A/B scripts
_lib = None

STAGE_FWD_COLUMNS, STAGE_FWD_ROWS, STAGE_POINTWISE, STAGE_INV_ROWS, STAGE_INV_COLUMNS, \
    STAGE_SCALE, STAGE_COMBINE, STAGE_FOLD_COMBINE = range(8)
STAGE_PRE_STORE = 8   # precomp_stage: operand B's row arrays -> the cache
# (tests) or-ed onto STAGE_INV_ROWS / _INV_COLUMNS / _SCALE: the stage as the whole multiply drives it
STAGE_DRIVEN = 0x100

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_L = ctypes.c_long
_UL = ctypes.c_ulong


class _Shard(ctypes.Structure):
    """struct mpfft_shard (include/mpfft.h)"""
    _fields_ = [("n1", ctypes.c_long), ("n2", ctypes.c_long), ("depth", ctypes.c_ulong), ("w", ctypes.c_ulong),
                ("c0", ctypes.c_int), ("ccount", ctypes.c_int), ("r0", ctypes.c_int), ("rcount", ctypes.c_int),
                ("ccb", ctypes.c_int),
                ("col_dig", ctypes.c_void_p * 2), ("col_cb", ctypes.c_void_p * 2), ("col_top", ctypes.c_void_p * 2),
                ("row_dig", ctypes.c_void_p * 2), ("row_cb", ctypes.c_void_p * 2), ("row_top", ctypes.c_void_p * 2),
                ("src_chunk", ctypes.c_long),
                ("rowc_dig", ctypes.c_void_p), ("rowc_cb", ctypes.c_void_p), ("rowc_top", ctypes.c_void_p)]


class _Copy(ctypes.Structure):
    """struct mpfft_copy (include/mpfft.h)"""
    _fields_ = [("src", ctypes.c_int), ("dst", ctypes.c_int), ("op", ctypes.c_int), ("field", ctypes.c_int),
                ("src_layout", ctypes.c_int), ("dst_layout", ctypes.c_int),
                ("src_off", ctypes.c_long), ("dst_off", ctypes.c_long), ("count", ctypes.c_long)]


XCHG_COL_TO_ROW, XCHG_ROW_TO_COL = 1, 2
LAYOUT_HALO = 2      # mpfft_copy.dst_layout of a halo copy


class MpfftError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: {strerror(code)} (code {code})")
        self.code = code


def lib():
    """The loaded libmpfft.so (raises if it was not built -- no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # One HIP runtime per process: torch ships its own libamdhip64 (same SONAME,
        # different file name).  Loading torch first makes libmpfft's NEEDED
        # libamdhip64.so.7 bind to that copy, so device pointers and streams from
        # torch are valid here; loading libmpfft first would pull in /opt/rocm's copy
        # and a later torch import would start a second runtime that sees no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        h = ctypes.CDLL(LIB_PATH)
        h.new_mpn_mul.argtypes = [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]
        h.new_mpn_mul.restype = None
        h.mpfft_mul_ex.argtypes = [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]
        h.mpfft_mul_ex.restype = ctypes.c_int
        h.mpfft_profile_begin.argtypes = [ctypes.c_int]
        h.mpfft_profile_begin.restype = ctypes.c_int
        h.mpfft_profile_end.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
        h.mpfft_profile_end.restype = ctypes.c_int
        h.mpfft_stage_kernels.argtypes = [_L, _L, _UL, _UL, ctypes.c_char_p, ctypes.c_size_t]
        h.mpfft_stage_kernels.restype = ctypes.c_int
        h.mpfft_release.argtypes = []
        h.mpfft_release.restype = ctypes.c_int
        h.mpfft_mul_device.argtypes = [_vp, _vp, _L, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
        h.mpfft_mul_device.restype = ctypes.c_int
        h.mpfft_stage.argtypes = [ctypes.c_int, _vp, _vp, _vp, _L, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
        h.mpfft_stage.restype = ctypes.c_int
        h.mpfft_workspace_bytes.argtypes = [_L, _L, _UL, _UL]
        h.mpfft_workspace_bytes.restype = ctypes.c_size_t
        h.mpfft_check_params.argtypes = [_L, _L, _UL, _UL]
        h.mpfft_check_params.restype = ctypes.c_int
        h.mpfft_plan_info.argtypes = [_L, _L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
        h.mpfft_plan_info.restype = ctypes.c_int
        h.mpfft_workspace_layout.argtypes = [_L, _L, _UL, _UL, ctypes.POINTER(ctypes.c_size_t)]
        h.mpfft_workspace_layout.restype = ctypes.c_int
        h.mpfft_strerror.argtypes = [ctypes.c_int]
        h.mpfft_strerror.restype = ctypes.c_char_p
        h.mpfft_version.argtypes = []
        h.mpfft_version.restype = ctypes.c_int
        h.mpfft_fill_random.argtypes = [_u64p, _L, ctypes.c_uint64]
        h.mpfft_fill_random.restype = None
        h.mpfft_shard_stage.argtypes = [ctypes.c_int, ctypes.POINTER(_Shard), _vp, _vp, _vp]
        h.mpfft_shard_stage.restype = ctypes.c_int
        h.mpfft_shard_stage_rows.argtypes = [ctypes.c_int, ctypes.POINTER(_Shard), ctypes.c_int, ctypes.c_int, _vp]
        h.mpfft_shard_stage_rows.restype = ctypes.c_int
        h.mpfft_shard_row_fused.argtypes = [_L, _L, _UL, _UL, ctypes.c_int]
        h.mpfft_shard_row_fused.restype = ctypes.c_int
        h.mpfft_shard_combine_tmp_bytes.argtypes = [_L, _L, _UL, _UL, ctypes.c_int]
        h.mpfft_shard_combine_tmp_bytes.restype = ctypes.c_size_t
        h.mpfft_shard_combine.argtypes = [ctypes.POINTER(_Shard), ctypes.c_int, _vp, _vp, _vp, _vp, _vp,
                                          ctypes.c_size_t, _vp]
        h.mpfft_shard_combine.restype = ctypes.c_int
        _lp = ctypes.POINTER(ctypes.c_long)
        h.mpfft_shard_partition.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, _lp, _lp]
        h.mpfft_shard_partition.restype = ctypes.c_int
        h.mpfft_shard_stripes.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, _lp, _L]
        h.mpfft_shard_stripes.restype = ctypes.c_long
        h.mpfft_shard_exchange_plan.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(_Copy), _L]
        h.mpfft_shard_exchange_plan.restype = ctypes.c_long
        h.mpfft_shard_halo_plan.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, ctypes.POINTER(_Copy), _L]
        h.mpfft_shard_halo_plan.restype = ctypes.c_long
        h.mpfft_shard_src_limbs.argtypes = [_L, _L, _UL, _UL, ctypes.c_int]
        h.mpfft_shard_src_limbs.restype = ctypes.c_long
        h.mpfft_shard_pack.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, ctypes.c_int, _u64p, _L, _u64p]
        h.mpfft_shard_pack.restype = ctypes.c_int
        h.mpfft_mul_multi_device.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                             ctypes.POINTER(_vp)]
        h.mpfft_mul_multi_device.restype = ctypes.c_int
        h.mpfft_mul_multi.argtypes = [_u64p, _u64p, _L, _u64p, _L, _UL, _UL, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
        h.mpfft_mul_multi.restype = ctypes.c_int
        h.mpfft_multi_release.argtypes = []
        h.mpfft_multi_release.restype = ctypes.c_int
        if hasattr(h, "mpfft_multi_schedule"):   # (older libraries in A/B runs lack it)
            h.mpfft_multi_schedule.argtypes = [_L, _L, _UL, _UL, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                               ctypes.c_size_t]
            h.mpfft_multi_schedule.restype = ctypes.c_long
        h.mpfft_set_devices.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), _L]
        h.mpfft_set_devices.restype = ctypes.c_int
        h.mpfft_last_ngpus.argtypes = []
        h.mpfft_last_ngpus.restype = ctypes.c_int
        h.mpfft_choose.argtypes = [_L, _L, ctypes.POINTER(ctypes.c_ulong), ctypes.POINTER(ctypes.c_ulong)]
        h.mpfft_choose.restype = ctypes.c_int
        h.mpfft_mul_auto.argtypes = [_u64p, _u64p, _L, _u64p, _L]
        h.mpfft_mul_auto.restype = ctypes.c_int
        h.new_mpn_mul6.argtypes = [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]
        h.new_mpn_mul6.restype = None
        h.mpfft_mul6_ex.argtypes = [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]
        h.mpfft_mul6_ex.restype = ctypes.c_int
        h.mpfft_mul6_device.argtypes = [_vp, _vp, _L, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
        h.mpfft_mul6_device.restype = ctypes.c_int
        h.mpfft_workspace_bytes6.argtypes = [_L, _L, _UL, _UL]
        h.mpfft_workspace_bytes6.restype = ctypes.c_size_t
        h.mpfft_check_params6.argtypes = [_L, _L, _UL, _UL]
        h.mpfft_check_params6.restype = ctypes.c_int
        h.mpfft_plan_info6.argtypes = [_L, _L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
        h.mpfft_plan_info6.restype = ctypes.c_int
        if hasattr(h, "mpfft_sqr_ex"):   # MPFFT_VERSION 3 (older libraries in A/B runs lack them)
            h.mpfft_sqr_ex.argtypes = [_u64p, _u64p, _L, _UL, _UL]
            h.mpfft_sqr_ex.restype = ctypes.c_int
            h.mpfft_sqr_auto.argtypes = [_u64p, _u64p, _L]
            h.mpfft_sqr_auto.restype = ctypes.c_int
            h.mpfft_sqr_device.argtypes = [_vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_sqr_device.restype = ctypes.c_int
            h.mpfft_sqr_workspace_bytes.argtypes = [_L, _UL, _UL]
            h.mpfft_sqr_workspace_bytes.restype = ctypes.c_size_t
            h.mpfft_sqr_workspace_layout.argtypes = [_L, _UL, _UL, ctypes.POINTER(ctypes.c_size_t)]
            h.mpfft_sqr_workspace_layout.restype = ctypes.c_int
            h.mpfft_sqr_stage.argtypes = [ctypes.c_int, _vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_sqr_stage.restype = ctypes.c_int
            h.mpfft_sqr_stage_kernels.argtypes = [_L, _UL, _UL, ctypes.c_char_p, ctypes.c_size_t]
            h.mpfft_sqr_stage_kernels.restype = ctypes.c_int
        if hasattr(h, "mpfft_mulmod_ex"):   # MPFFT_VERSION 4 (older libraries in A/B runs lack them)
            _ulp = ctypes.POINTER(ctypes.c_ulong)
            h.mpfft_mulmod_check_params.argtypes = [_L, _UL, _UL]
            h.mpfft_mulmod_check_params.restype = ctypes.c_int
            h.mpfft_mulmod_ex.argtypes = [_u64p, _u64p, _u64p, _L, _UL, _UL]
            h.mpfft_mulmod_ex.restype = ctypes.c_int
            h.mpfft_sqrmod_ex.argtypes = [_u64p, _u64p, _L, _UL, _UL]
            h.mpfft_sqrmod_ex.restype = ctypes.c_int
            h.mpfft_mulmod_device.argtypes = [_vp, _vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_mulmod_device.restype = ctypes.c_int
            h.mpfft_sqrmod_device.argtypes = [_vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_sqrmod_device.restype = ctypes.c_int
            h.mpfft_mulmod_workspace_bytes.argtypes = [_L, _UL, _UL, ctypes.c_int]
            h.mpfft_mulmod_workspace_bytes.restype = ctypes.c_size_t
            h.mpfft_mulmod_plan_info.argtypes = [_L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
            h.mpfft_mulmod_plan_info.restype = ctypes.c_int
            h.mpfft_mulmod_workspace_layout.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
            h.mpfft_mulmod_workspace_layout.restype = ctypes.c_int
            h.mpfft_mulmod_stage.argtypes = [ctypes.c_int, _vp, _vp, _vp, _L, _UL, _UL, ctypes.c_int, _vp,
                                             ctypes.c_size_t, _vp]
            h.mpfft_mulmod_stage.restype = ctypes.c_int
            h.mpfft_mulmod_stage_kernels.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
            h.mpfft_mulmod_stage_kernels.restype = ctypes.c_int
            h.mpfft_mulmod_choose.argtypes = [_L, _ulp, _ulp]
            h.mpfft_mulmod_choose.restype = ctypes.c_int
            h.mpfft_mulmod_next_size.argtypes = [_L, ctypes.POINTER(ctypes.c_long), _ulp, _ulp]
            h.mpfft_mulmod_next_size.restype = ctypes.c_int
        if hasattr(h, "mpfft_precomp_device"):   # MPFFT_VERSION 5 (older libraries in A/B runs lack them)
            _sz = ctypes.c_size_t
            h.mpfft_precomp_bytes.argtypes = [_L, _L, _UL, _UL]
            h.mpfft_precomp_bytes.restype = _sz
            h.mpfft_precomp_device.argtypes = [_vp, _sz, _vp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_precomp_device.restype = ctypes.c_int
            h.mpfft_mul_precomp_workspace_bytes.argtypes = [_L, _L, _UL, _UL]
            h.mpfft_mul_precomp_workspace_bytes.restype = _sz
            h.mpfft_mul_precomp_device.argtypes = [_vp, _vp, _L, _vp, _sz, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_mul_precomp_device.restype = ctypes.c_int
            h.mpfft_precomp_stage_kernels.argtypes = [_L, _L, _UL, _UL, ctypes.c_char_p, _sz]
            h.mpfft_precomp_stage_kernels.restype = ctypes.c_int
            h.mpfft_precomp_stage.argtypes = [ctypes.c_int, _vp, _sz, _vp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_precomp_stage.restype = ctypes.c_int
            h.mpfft_mul_precomp_stage.argtypes = [ctypes.c_int, _vp, _vp, _sz, _vp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_mul_precomp_stage.restype = ctypes.c_int
            h.mpfft_precomp_create.argtypes = [ctypes.POINTER(_vp), _u64p, _L, _L, _UL, _UL]
            h.mpfft_precomp_create.restype = ctypes.c_int
            h.mpfft_mul_precomp_ex.argtypes = [_u64p, _u64p, _L, _vp]
            h.mpfft_mul_precomp_ex.restype = ctypes.c_int
            h.mpfft_precomp_destroy.argtypes = [_vp]
            h.mpfft_precomp_destroy.restype = None
        if hasattr(h, "mpfft_mulmodm1_ex"):   # MPFFT_VERSION 6 (older libraries in A/B runs lack them)
            _ulp = ctypes.POINTER(ctypes.c_ulong)
            _sz = ctypes.c_size_t
            h.mpfft_mulmodm1_check_params.argtypes = [_L, _UL, _UL]
            h.mpfft_mulmodm1_check_params.restype = ctypes.c_int
            h.mpfft_mulmodm1_ex.argtypes = [_u64p, _u64p, _u64p, _L, _UL, _UL]
            h.mpfft_mulmodm1_ex.restype = ctypes.c_int
            h.mpfft_sqrmodm1_ex.argtypes = [_u64p, _u64p, _L, _UL, _UL]
            h.mpfft_sqrmodm1_ex.restype = ctypes.c_int
            h.mpfft_mulmodm1_device.argtypes = [_vp, _vp, _vp, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_mulmodm1_device.restype = ctypes.c_int
            h.mpfft_sqrmodm1_device.argtypes = [_vp, _vp, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_sqrmodm1_device.restype = ctypes.c_int
            h.mpfft_mulmodm1_workspace_bytes.argtypes = [_L, _UL, _UL, ctypes.c_int]
            h.mpfft_mulmodm1_workspace_bytes.restype = _sz
            h.mpfft_mulmodm1_plan_info.argtypes = [_L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
            h.mpfft_mulmodm1_plan_info.restype = ctypes.c_int
            h.mpfft_mulmodm1_workspace_layout.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.POINTER(_sz)]
            h.mpfft_mulmodm1_workspace_layout.restype = ctypes.c_int
            h.mpfft_mulmodm1_stage.argtypes = [ctypes.c_int, _vp, _vp, _vp, _L, _UL, _UL, ctypes.c_int, _vp, _sz, _vp]
            h.mpfft_mulmodm1_stage.restype = ctypes.c_int
            h.mpfft_mulmodm1_stage_kernels.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.c_char_p, _sz]
            h.mpfft_mulmodm1_stage_kernels.restype = ctypes.c_int
            h.mpfft_mulmodm1_choose.argtypes = [_L, _ulp, _ulp]
            h.mpfft_mulmodm1_choose.restype = ctypes.c_int
            h.mpfft_mulmodm1_next_size.argtypes = [_L, ctypes.POINTER(ctypes.c_long), _ulp, _ulp]
            h.mpfft_mulmodm1_next_size.restype = ctypes.c_int
            h.mpfft_mulmodm1_precomp_bytes.argtypes = [_L, _UL, _UL]
            h.mpfft_mulmodm1_precomp_bytes.restype = _sz
            h.mpfft_mulmodm1_precomp_device.argtypes = [_vp, _sz, _vp, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_mulmodm1_precomp_device.restype = ctypes.c_int
            h.mpfft_mulmodm1_mul_precomp_device.argtypes = [_vp, _vp, _vp, _sz, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_mulmodm1_mul_precomp_device.restype = ctypes.c_int
        if hasattr(h, "mpfft_mulmodw_ex"):   # MPFFT_VERSION 7 (older libraries in A/B runs lack them)
            _ulp = ctypes.POINTER(ctypes.c_ulong)
            h.mpfft_mulmodw_check_params.argtypes = [_L, _UL, _UL]
            h.mpfft_mulmodw_check_params.restype = ctypes.c_int
            h.mpfft_mulmodw_ex.argtypes = [_u64p, _u64p, _u64p, _L, _UL, _UL]
            h.mpfft_mulmodw_ex.restype = ctypes.c_int
            h.mpfft_sqrmodw_ex.argtypes = [_u64p, _u64p, _L, _UL, _UL]
            h.mpfft_sqrmodw_ex.restype = ctypes.c_int
            h.mpfft_mulmodw_device.argtypes = [_vp, _vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_mulmodw_device.restype = ctypes.c_int
            h.mpfft_sqrmodw_device.argtypes = [_vp, _vp, _L, _UL, _UL, _vp, ctypes.c_size_t, _vp]
            h.mpfft_sqrmodw_device.restype = ctypes.c_int
            h.mpfft_mulmodw_workspace_bytes.argtypes = [_L, _UL, _UL, ctypes.c_int]
            h.mpfft_mulmodw_workspace_bytes.restype = ctypes.c_size_t
            h.mpfft_mulmodw_plan_info.argtypes = [_L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
            h.mpfft_mulmodw_plan_info.restype = ctypes.c_int
            h.mpfft_mulmodw_workspace_layout.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
            h.mpfft_mulmodw_workspace_layout.restype = ctypes.c_int
            h.mpfft_mulmodw_stage.argtypes = [ctypes.c_int, _vp, _vp, _vp, _L, _UL, _UL, ctypes.c_int, _vp,
                                              ctypes.c_size_t, _vp]
            h.mpfft_mulmodw_stage.restype = ctypes.c_int
            h.mpfft_mulmodw_stage_kernels.argtypes = [_L, _UL, _UL, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
            h.mpfft_mulmodw_stage_kernels.restype = ctypes.c_int
            h.mpfft_mulmodw_choose.argtypes = [_L, _ulp, _ulp]
            h.mpfft_mulmodw_choose.restype = ctypes.c_int
            h.mpfft_mulmodw_next_size.argtypes = [_L, ctypes.POINTER(ctypes.c_long), _ulp, _ulp]
            h.mpfft_mulmodw_next_size.restype = ctypes.c_int
        if hasattr(h, "mpfft_dot_device"):   # MPFFT_VERSION 8 (older libraries in A/B runs lack them)
            _ulp = ctypes.POINTER(ctypes.c_ulong)
            _sz = ctypes.c_size_t
            _pp = ctypes.POINTER(ctypes.c_void_p)
            h.mpfft_dot_check_params.argtypes = [_L, _L, _L, _UL, _UL]
            h.mpfft_dot_check_params.restype = ctypes.c_int
            h.mpfft_dot_plan_info.argtypes = [_L, _L, _L, _UL, _UL, ctypes.POINTER(ctypes.c_long)]
            h.mpfft_dot_plan_info.restype = ctypes.c_int
            h.mpfft_dot_choose.argtypes = [_L, _L, _L, _ulp, _ulp]
            h.mpfft_dot_choose.restype = ctypes.c_int
            h.mpfft_dot_workspace_bytes.argtypes = [_L, _L, _L, _UL, _UL]
            h.mpfft_dot_workspace_bytes.restype = _sz
            h.mpfft_dot_workspace_layout.argtypes = [_L, _L, _L, _UL, _UL, ctypes.POINTER(_sz)]
            h.mpfft_dot_workspace_layout.restype = ctypes.c_int
            h.mpfft_dot_device.argtypes = [_vp, _L, _pp, _pp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_dot_device.restype = ctypes.c_int
            h.mpfft_dot_ex.argtypes = [_u64p, _L, _pp, _pp, _L, _L, _UL, _UL]
            h.mpfft_dot_ex.restype = ctypes.c_int
            h.mpfft_dot_auto.argtypes = [_u64p, _L, _pp, _pp, _L, _L]
            h.mpfft_dot_auto.restype = ctypes.c_int
            h.mpfft_dot_stage_kernels.argtypes = [_L, _L, _L, _UL, _UL, ctypes.c_char_p, _sz]
            h.mpfft_dot_stage_kernels.restype = ctypes.c_int
            h.mpfft_dot_stage.argtypes = [ctypes.c_int, _L, _vp, _vp, _vp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_dot_stage.restype = ctypes.c_int
        if hasattr(h, "mpfft_sdot_device"):   # MPFFT_VERSION 9
            _sz = ctypes.c_size_t
            _pp = ctypes.POINTER(ctypes.c_void_p)
            _U64 = ctypes.c_uint64
            h.mpfft_sdot_check_params.argtypes = [_L, _U64, _L, _L, _UL, _UL]
            h.mpfft_sdot_check_params.restype = ctypes.c_int
            h.mpfft_sdot_workspace_bytes.argtypes = [_L, _L, _L, _UL, _UL]
            h.mpfft_sdot_workspace_bytes.restype = _sz
            h.mpfft_sdot_workspace_layout.argtypes = [_L, _L, _L, _UL, _UL, ctypes.POINTER(_sz)]
            h.mpfft_sdot_workspace_layout.restype = ctypes.c_int
            h.mpfft_sdot_device.argtypes = [_vp, _L, _U64, _pp, _pp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_sdot_device.restype = ctypes.c_int
            h.mpfft_sdot_ex.argtypes = [_u64p, _L, _U64, _pp, _pp, _L, _L, _UL, _UL]
            h.mpfft_sdot_ex.restype = ctypes.c_int
            h.mpfft_sdot_auto.argtypes = [_u64p, _L, _U64, _pp, _pp, _L, _L]
            h.mpfft_sdot_auto.restype = ctypes.c_int
            h.mpfft_sdot_stage_kernels.argtypes = [_L, _U64, _L, _L, _UL, _UL, ctypes.c_char_p, _sz]
            h.mpfft_sdot_stage_kernels.restype = ctypes.c_int
            h.mpfft_sdot_stage.argtypes = [ctypes.c_int, _L, _vp, _vp, _vp, _L, _L, _UL, _UL, _vp, _sz, _vp]
            h.mpfft_sdot_stage.restype = ctypes.c_int
        _lib = h
    return _lib


def strerror(code):
    return lib().mpfft_strerror(int(code)).decode()


def _p(a):
    if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("limb arrays must be C-contiguous numpy.uint64")
    return a.ctypes.data_as(_u64p)


def check_params(n1, n2, depth, w):
    return lib().mpfft_check_params(n1, n2, depth, w)


def plan_info(n1, n2, depth, w):
    """dict of the derived parameters (mul_fft.c:3193-3203) or MpfftError."""
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_plan_info(n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, f"plan(n1={n1}, n2={n2}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def workspace_bytes(n1, n2, depth, w):
    return int(lib().mpfft_workspace_bytes(n1, n2, depth, w))


def new_mpn_mul(r1, i1, n1, i2, n2, depth, w):
    """Reference-shaped entry (mul_fft.c:3190): r1[:n1+n2] = i1[:n1] * i2[:n2]."""
    if len(r1) < n1 + n2 or len(i1) < n1 or len(i2) < n2:
        raise ValueError("buffer shorter than the stated limb count")
    rc = lib().mpfft_mul_ex(_p(r1), _p(i1), n1, _p(i2), n2, depth, w)
    if rc:
        raise MpfftError(rc, f"new_mpn_mul(n1={n1}, n2={n2}, depth={depth}, w={w})")


def mul(i1, i2, depth, w):
    """Convenience: returns the n1+n2 limb product as a new uint64 array."""
    i1 = np.ascontiguousarray(i1, dtype=np.uint64)
    i2 = np.ascontiguousarray(i2, dtype=np.uint64)
    r = np.zeros(len(i1) + len(i2), dtype=np.uint64)
    new_mpn_mul(r, i1, len(i1), i2, len(i2), depth, w)
    return r


def choose(n1, n2):
    """(depth, w) the library would use for an n1 x n2-limb product (mpfft_choose: the
    reference leaves them to the caller, mul_fft.c:3190-3191)."""
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_choose(n1, n2, ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"choose(n1={n1}, n2={n2})")
    return int(d.value), int(w.value)


def mul_auto(i1, i2):
    """mpn_mul-style product with (depth, w) from choose(): a new uint64 array of n1+n2 limbs."""
    i1 = np.ascontiguousarray(i1, dtype=np.uint64)
    i2 = np.ascontiguousarray(i2, dtype=np.uint64)
    r = np.zeros(len(i1) + len(i2), dtype=np.uint64)
    rc = lib().mpfft_mul_auto(_p(r), _p(i1), len(i1), _p(i2), len(i2))
    if rc:
        raise MpfftError(rc, f"mul_auto(n1={len(i1)}, n2={len(i2)})")
    return r


# ---- the sqrt2 front end (new_mpn_mul6, mul_fft.c:3573-3668) --------------------------

def check_params6(n1, n2, depth, w):
    return lib().mpfft_check_params6(n1, n2, depth, w)


def plan_info6(n1, n2, depth, w):
    """derived parameters of new_mpn_mul6 (mul_fft.c:3575-3603): bits1 = (N - depth - 1)/2,
    trunc over a length-4n convolution"""
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_plan_info6(n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, f"plan6(n1={n1}, n2={n2}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def workspace_bytes6(n1, n2, depth, w):
    return int(lib().mpfft_workspace_bytes6(n1, n2, depth, w))


def new_mpn_mul6(r1, i1, n1, i2, n2, depth, w):
    """Reference-shaped entry (mul_fft.c:3573): r1[:n1+n2] = i1[:n1] * i2[:n2] through the
    sqrt2 transforms (length 4n, root sqrt2^w)"""
    if len(r1) < n1 + n2 or len(i1) < n1 or len(i2) < n2:
        raise ValueError("buffer shorter than the stated limb count")
    rc = lib().mpfft_mul6_ex(_p(r1), _p(i1), n1, _p(i2), n2, depth, w)
    if rc:
        raise MpfftError(rc, f"new_mpn_mul6(n1={n1}, n2={n2}, depth={depth}, w={w})")


def mul6(i1, i2, depth, w):
    i1 = np.ascontiguousarray(i1, dtype=np.uint64)
    i2 = np.ascontiguousarray(i2, dtype=np.uint64)
    r = np.zeros(len(i1) + len(i2), dtype=np.uint64)
    new_mpn_mul6(r, i1, len(i1), i2, len(i2), depth, w)
    return r


def alloc_workspace6(n1, n2, depth, w, device="cuda"):
    import torch
    nb = workspace_bytes6(n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(check_params6(n1, n2, depth, w), "workspace6")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mul6_device(d_r, d_i1, n1, d_i2, n2, depth, w, ws, stream=None):
    """new_mpn_mul6 on HBM-resident operands; queued on `stream`, not synchronised."""
    rc = lib().mpfft_mul6_device(_ptr(d_r), _ptr(d_i1), n1, _ptr(d_i2), n2, depth, w, _ptr(ws),
                                 ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mul6_device")


def fill_random(count, seed):
    buf = np.empty(count, dtype=np.uint64)
    lib().mpfft_fill_random(_p(buf), count, seed)
    return buf


# ---- device-resident entry points (torch tensors as HBM plumbing) ----------

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def alloc_workspace(n1, n2, depth, w, device="cuda"):
    import torch
    nb = workspace_bytes(n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(check_params(n1, n2, depth, w), "workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mul_device(d_r, d_i1, n1, d_i2, n2, depth, w, ws, stream=None):
    """All tensors on the GPU (int64/uint64 limbs); queued on `stream`, not synchronised."""
    rc = lib().mpfft_mul_device(_ptr(d_r), _ptr(d_i1), n1, _ptr(d_i2), n2, depth, w, _ptr(ws),
                                ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mul_device")


def stage(which, d_i1, d_i2, d_r, n1, n2, depth, w, ws, stream=None):
    rc = lib().mpfft_stage(which, _ptr(d_i1), _ptr(d_i2), _ptr(d_r), n1, n2, depth, w, _ptr(ws),
                           ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_stage({which})")


STAGE_NAMES = ("fwd_columns", "fwd_rows", "pointwise", "inv_rows", "inv_columns", "scale", "combine")


def stage_kernels(n1, n2, depth, w):
    """dict stage -> the kernel the library launches for it with these parameters"""
    buf = ctypes.create_string_buffer(512)
    rc = lib().mpfft_stage_kernels(n1, n2, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


def inv_columns_schedule(n1, n2, depth, w):
    """The launches of the single-device truncated inverse column transform, in order (a host-side
    dry run: needs no GPU)."""
    f = lib().mpfft_inv_columns_schedule
    f.argtypes = [_L, _L, _UL, _UL, ctypes.c_char_p, ctypes.c_size_t]
    f.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(1 << 16)
    rc = f(n1, n2, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_inv_columns_schedule")
    return buf.value.decode().splitlines()


def profile_begin(max_calls):
    """Record HIP events at the stage boundaries of the next max_calls multiplies."""
    rc = lib().mpfft_profile_begin(max_calls)
    if rc:
        raise MpfftError(rc, "mpfft_profile_begin")


def profile_end():
    """(dict stage -> summed ms, number of profiled multiplies); synchronises."""
    ms = (ctypes.c_float * len(STAGE_NAMES))()
    calls = ctypes.c_int(0)
    rc = lib().mpfft_profile_end(ms, ctypes.byref(calls))
    if rc:
        raise MpfftError(rc, "mpfft_profile_end")
    return dict(zip(STAGE_NAMES, [float(x) for x in ms])), calls.value


def workspace_layout(n1, n2, depth, w):
    out = (ctypes.c_size_t * 8)()
    rc = lib().mpfft_workspace_layout(n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, "workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw")
    return dict(zip(keys, list(out)))


def workspace_views(ws, n1, n2, depth, w):
    """(digA, topA, digB, topB) views into a single-GPU workspace tensor (slot-major).
    Only meaningful for canonically stored stages (carry masks zero)."""
    import torch
    P = plan_info(n1, n2, depth, w)
    lay = workspace_layout(n1, n2, depth, w)
    slots, l = lay["slots"], P["l"]
    u8 = ws.view(torch.uint8)

    def dig(off):
        return u8[off:off + slots * l * 8].view(torch.int64).view(slots, l)

    def top(off):
        return u8[off:off + slots * 4].view(torch.int32)
    return dig(lay["digA"]), top(lay["topA"]), dig(lay["digB"]), top(lay["topB"])


# ---- squaring (mpfft_sqr_*, include/mpfft.h): one operand, no B arrays in the workspace ----

def sqr(a, depth, w):
    """The 2n-limb square of `a` as a new uint64 array (host pointers, mpfft_sqr_ex)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    r = np.zeros(2 * len(a), dtype=np.uint64)
    rc = lib().mpfft_sqr_ex(_p(r), _p(a), len(a), depth, w)
    if rc:
        raise MpfftError(rc, f"sqr(n={len(a)}, depth={depth}, w={w})")
    return r


def sqr_auto(a):
    """mpn_sqr-style square with (depth, w) from choose(n, n)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    r = np.zeros(2 * len(a), dtype=np.uint64)
    rc = lib().mpfft_sqr_auto(_p(r), _p(a), len(a))
    if rc:
        raise MpfftError(rc, f"sqr_auto(n={len(a)})")
    return r


def sqr_workspace_bytes(n, depth, w):
    return int(lib().mpfft_sqr_workspace_bytes(n, depth, w))


def alloc_workspace_sqr(n, depth, w, device="cuda"):
    import torch
    nb = sqr_workspace_bytes(n, depth, w)
    if nb == 0:
        raise MpfftError(check_params(n, n, depth, w), "sqr workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def sqr_device(d_r, d_a, n, depth, w, ws, stream=None):
    """d_r[:2n] = d_a[:n]^2, all tensors on the GPU; queued on `stream`, not synchronised."""
    rc = lib().mpfft_sqr_device(_ptr(d_r), _ptr(d_a), n, depth, w, _ptr(ws),
                                ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_sqr_device")


def sqr_stage(which, d_a, d_r, n, depth, w, ws, stream=None):
    rc = lib().mpfft_sqr_stage(which, _ptr(d_a), _ptr(d_r), n, depth, w, _ptr(ws),
                               ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_sqr_stage({which})")


def sqr_stage_kernels(n, depth, w):
    """dict stage -> the kernel a square launches for it (the pointwise: k_pwsq<M>... or
    '<kernel> (B = A)')"""
    buf = ctypes.create_string_buffer(512)
    rc = lib().mpfft_sqr_stage_kernels(n, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_sqr_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


def sqr_workspace_layout(n, depth, w):
    out = (ctypes.c_size_t * 8)()
    rc = lib().mpfft_sqr_workspace_layout(n, depth, w, out)
    if rc:
        raise MpfftError(rc, "sqr_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw")
    return dict(zip(keys, list(out)))


def sqr_workspace_views(ws, n, depth, w):
    """(digA, topA) views into a square's workspace tensor (slot-major), as workspace_views."""
    import torch
    P = plan_info(n, n, depth, w)
    lay = sqr_workspace_layout(n, depth, w)
    slots, l = lay["slots"], P["l"]
    u8 = ws.view(torch.uint8)
    dig = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
    top = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
    return dig, top


# ---- sums of products (mpfft_dot_*, include/mpfft.h): r = sum_i a_i b_i with K forward transform
# pairs and one inverse; the workspace has a third coefficient array C, the accumulator ----

DOT_MAX = 64
STAGE_ACC = 0x200   # dot_stage: or-ed onto STAGE_POINTWISE, C <- C + A B


def dot_check_params(K, n1, n2, depth, w):
    return lib().mpfft_dot_check_params(K, n1, n2, depth, w)


def dot_plan_info(K, n1, n2, depth, w):
    """plan_info of a K-term sum: bits1 = (N - depth - ceil(log2 K)) / 2 and what follows from it"""
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_dot_plan_info(K, n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, f"dot plan(K={K}, n1={n1}, n2={n2}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def dot_choose(K, n1, n2):
    """(depth, w) the library would use for a K-term sum of n1 x n2-limb products"""
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_dot_choose(K, n1, n2, ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"dot_choose(K={K}, n1={n1}, n2={n2})")
    return int(d.value), int(w.value)


def dot_max_limbs(K, depth, w):
    """largest n with n1 = n2 = n valid for a K-term sum at (depth, w): j1 = j2 = 2^depth pieces of
    bits1 = (N - depth - ceil(log2 K)) / 2 bits"""
    N = (1 << depth) * w
    bits1 = (N - depth - (K - 1).bit_length()) // 2
    return (1 << depth) * bits1 // 64


def dot_workspace_bytes(K, n1, n2, depth, w):
    return int(lib().mpfft_dot_workspace_bytes(K, n1, n2, depth, w))


def alloc_workspace_dot(K, n1, n2, depth, w, device="cuda"):
    import torch
    nb = dot_workspace_bytes(K, n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(dot_check_params(K, n1, n2, depth, w), "dot workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def dot_workspace_layout(K, n1, n2, depth, w):
    out = (ctypes.c_size_t * 11)()
    rc = lib().mpfft_dot_workspace_layout(K, n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, "dot_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw", "digC", "topC", "cbC")
    return dict(zip(keys, list(out)))


def dot_workspace_views(ws, K, n1, n2, depth, w):
    """{"A", "B", "C"} -> (dig, top, cb) views into a dot workspace tensor (slot-major): limbs
    (slots, l) int64, carry limbs int32, carry-mask words (slots, cbw) int64"""
    import torch
    P = dot_plan_info(K, n1, n2, depth, w)
    lay = dot_workspace_layout(K, n1, n2, depth, w)
    slots, l, cbw = lay["slots"], P["l"], lay["cbw"]
    u8 = ws.view(torch.uint8)

    def arrays(x):
        d, t, c = lay["dig" + x], lay["top" + x], lay["cb" + x]
        return (u8[d:d + slots * l * 8].view(torch.int64).view(slots, l), u8[t:t + slots * 4].view(torch.int32),
                u8[c:c + slots * cbw * 8].view(torch.int64).view(slots, cbw))
    return {x: arrays(x) for x in "ABC"}


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def dot_device(d_r, d_as, d_bs, n1, n2, depth, w, ws, stream=None):
    """d_r[:n1 + n2 + 1] = sum_i d_as[i][:n1] * d_bs[i][:n2], all tensors on the GPU (lists of K
    tensors; the same tensor may appear more than once); queued on `stream`, not synchronised."""
    if len(d_as) != len(d_bs):
        raise ValueError("as many a_i as b_i")
    rc = lib().mpfft_dot_device(_ptr(d_r), len(d_as), _ptr_array(d_as), _ptr_array(d_bs), n1, n2, depth, w, _ptr(ws),
                                ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_dot_device")


def _host_terms(a_list, b_list):
    a_list = [np.ascontiguousarray(a, dtype=np.uint64) for a in a_list]
    b_list = [np.ascontiguousarray(b, dtype=np.uint64) for b in b_list]
    if len(a_list) != len(b_list) or not a_list:
        raise ValueError("as many a_i as b_i, at least one")
    n1, n2 = len(a_list[0]), len(b_list[0])
    if any(len(a) != n1 for a in a_list) or any(len(b) != n2 for b in b_list):
        raise ValueError("every a_i of n1 limbs, every b_i of n2 limbs")
    pa = (ctypes.c_void_p * len(a_list))(*[a.ctypes.data for a in a_list])
    pb = (ctypes.c_void_p * len(b_list))(*[b.ctypes.data for b in b_list])
    return a_list, b_list, pa, pb, n1, n2


def dot(a_list, b_list, depth, w):
    """sum_i a_list[i] * b_list[i] as a new uint64 array of n1 + n2 + 1 limbs (host pointers, mpfft_dot_ex)"""
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    rc = lib().mpfft_dot_ex(_p(r), len(a_list), pa, pb, n1, n2, depth, w)
    if rc:
        raise MpfftError(rc, f"dot(K={len(a_list)}, n1={n1}, n2={n2}, depth={depth}, w={w})")
    return r


def dot_auto(a_list, b_list):
    """dot() with (depth, w) from dot_choose()"""
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    rc = lib().mpfft_dot_auto(_p(r), len(a_list), pa, pb, n1, n2)
    if rc:
        raise MpfftError(rc, f"dot_auto(K={len(a_list)}, n1={n1}, n2={n2})")
    return r


def dot_stage(which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream=None):
    """one stage for one term (d_a, d_b) on the K-term plan and workspace (tests)"""
    rc = lib().mpfft_dot_stage(which, K, _ptr(d_a), _ptr(d_b), _ptr(d_r), n1, n2, depth, w, _ptr(ws),
                               ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_dot_stage({which})")


def dot_stage_kernels(K, n1, n2, depth, w):
    """dict stage -> the kernels a K-term sum launches for it (the pointwise: the first term's kernel
    + the later terms')"""
    buf = ctypes.create_string_buffer(640)
    rc = lib().mpfft_dot_stage_kernels(K, n1, n2, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_dot_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


# ---- signed sums of products (mpfft_sdot_*, include/mpfft.h): r = sum_i +-a_i b_i on the dot plan
# (dot_choose, dot_plan_info, dot_max_limbs); the workspace is the dot's followed by the complement
# scratch and the accumulator D of the subtracted b_i ----

STAGE_SD_NEG = 10   # sdot_stage: d_a -> complement scratch, D <- d_b (| STAGE_ACC: D <- D + d_b)
STAGE_SD_FIX = 11   # sdot_stage: d_r <- d_r + D - (D << 64 n1)
SDOT_FIX_BLOCK = 4096   # limbs per block of the correction's carry chain (MPFFT_SDOT_FIX_BLOCK)


def _neg_mask(neg):
    """the sign mask as an int: an int is taken as it is, a sequence of booleans gives bit i = neg[i]"""
    if isinstance(neg, (int, np.integer)) and not isinstance(neg, (bool, np.bool_)):
        neg = int(neg)
    else:
        neg = sum(1 << i for i, x in enumerate(neg) if x)
    if neg < 0 or neg >> 64:
        raise ValueError("neg is a 64-bit mask")
    return neg


def sdot_to_int(limbs):
    """the signed Python integer of a two's-complement little-endian limb array"""
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
    v = int.from_bytes(limbs.tobytes(), "little")
    return v - (1 << (64 * len(limbs))) if len(limbs) and int(limbs[-1]) >> 63 else v


def sdot_check_params(K, neg, n1, n2, depth, w):
    return lib().mpfft_sdot_check_params(K, _neg_mask(neg), n1, n2, depth, w)


def sdot_workspace_bytes(K, n1, n2, depth, w):
    return int(lib().mpfft_sdot_workspace_bytes(K, n1, n2, depth, w))


def alloc_workspace_sdot(K, n1, n2, depth, w, device="cuda"):
    import torch
    nb = sdot_workspace_bytes(K, n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(dot_check_params(K, n1, n2, depth, w), "sdot workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def sdot_workspace_layout(K, n1, n2, depth, w):
    """dot_workspace_layout's entries, then "scratch" (the complement, n1 limbs) and "D" (n2 limbs)"""
    out = (ctypes.c_size_t * 13)()
    rc = lib().mpfft_sdot_workspace_layout(K, n1, n2, depth, w, out)
    if rc:
        raise MpfftError(rc, "sdot_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw", "digC", "topC", "cbC", "scratch", "D")
    return dict(zip(keys, list(out)))


def sdot_device(d_r, d_as, d_bs, neg, n1, n2, depth, w, ws, stream=None):
    """d_r[:n1 + n2 + 1] = sum_i +-d_as[i][:n1] * d_bs[i][:n2] in two's complement, term i subtracted
    where neg (an int mask or a sequence of booleans) says so; as dot_device otherwise."""
    if len(d_as) != len(d_bs):
        raise ValueError("as many a_i as b_i")
    rc = lib().mpfft_sdot_device(_ptr(d_r), len(d_as), _neg_mask(neg), _ptr_array(d_as), _ptr_array(d_bs), n1, n2, depth, w,
                                 _ptr(ws), ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_sdot_device")


def sdot(a_list, b_list, neg, depth, w):
    """sum_i +-a_list[i] * b_list[i] as a new uint64 array of n1 + n2 + 1 limbs, two's complement
    (host pointers, mpfft_sdot_ex); sdot_to_int gives its signed value"""
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    rc = lib().mpfft_sdot_ex(_p(r), len(a_list), _neg_mask(neg), pa, pb, n1, n2, depth, w)
    if rc:
        raise MpfftError(rc, f"sdot(K={len(a_list)}, n1={n1}, n2={n2}, depth={depth}, w={w})")
    return r


def sdot_auto(a_list, b_list, neg):
    """sdot() with (depth, w) from dot_choose()"""
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    rc = lib().mpfft_sdot_auto(_p(r), len(a_list), _neg_mask(neg), pa, pb, n1, n2)
    if rc:
        raise MpfftError(rc, f"sdot_auto(K={len(a_list)}, n1={n1}, n2={n2})")
    return r


def sdot_stage(which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream=None):
    """one stage on the signed sum's workspace (tests): STAGE_SD_NEG, STAGE_SD_FIX, or a dot_stage stage"""
    rc = lib().mpfft_sdot_stage(which, K, _ptr(d_a), _ptr(d_b), _ptr(d_r), n1, n2, depth, w, _ptr(ws),
                                ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_sdot_stage({which})")


def sdot_stage_kernels(K, neg, n1, n2, depth, w):
    """dot_stage_kernels' dict; with a negative term fwd_columns starts with the pre-pass kernel and
    combine ends with the correction's"""
    buf = ctypes.create_string_buffer(768)
    rc = lib().mpfft_sdot_stage_kernels(K, _neg_mask(neg), n1, n2, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_sdot_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


# ---- multiplication by a precomputed operand (mpfft_precomp_*, mpfft_mul_precomp_*, include/mpfft.h):
# operand 2's forward transform is computed once into a cache, bound to (n1, n2, depth, w) ----

def precomp_bytes(n1, n2, depth, w):
    return int(lib().mpfft_precomp_bytes(n1, n2, depth, w))


def alloc_precomp(n1, n2, depth, w, device="cuda"):
    import torch
    nb = precomp_bytes(n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(check_params(n1, n2, depth, w), "precomp cache")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def _nbytes(t):
    return t.numel() * t.element_size()


def precomp_device(pre, d_i2, n1, n2, depth, w, ws, stream=None):
    """d_i2[:n2] -> the cache `pre` (alloc_precomp) for products with n1-limb operands; ws is the
    multiply's workspace (alloc_workspace); queued on `stream`, not synchronised."""
    rc = lib().mpfft_precomp_device(_ptr(pre), _nbytes(pre), _ptr(d_i2), n1, n2, depth, w, _ptr(ws), _nbytes(ws),
                                    _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_precomp_device")


def mul_precomp_workspace_bytes(n1, n2, depth, w):
    return int(lib().mpfft_mul_precomp_workspace_bytes(n1, n2, depth, w))


def alloc_workspace_mul_precomp(n1, n2, depth, w, device="cuda"):
    import torch
    nb = mul_precomp_workspace_bytes(n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(check_params(n1, n2, depth, w), "mul_precomp workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mul_precomp_device(d_r, d_i1, n1, pre, n2, depth, w, ws, stream=None):
    """d_r[:n1+n2] = d_i1[:n1] * the operand cached in `pre` (only read); ws from
    alloc_workspace_mul_precomp; queued on `stream`, not synchronised."""
    rc = lib().mpfft_mul_precomp_device(_ptr(d_r), _ptr(d_i1), n1, _ptr(pre), _nbytes(pre), n2, depth, w, _ptr(ws),
                                        _nbytes(ws), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mul_precomp_device")


PRECOMP_STAGE_NAMES = ("precomp",) + STAGE_NAMES


def precomp_stage_kernels(n1, n2, depth, w):
    """dict: 'precomp' -> what writes the cache (k_pwsx<M>... or 'copy'), then stage -> the kernel a
    multiply against the cache launches (the pointwise: k_pwsp<M>... or '<kernel> (B cached)')"""
    buf = ctypes.create_string_buffer(640)
    rc = lib().mpfft_precomp_stage_kernels(n1, n2, depth, w, buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_precomp_stage_kernels")
    return dict(zip(PRECOMP_STAGE_NAMES, buf.value.decode().split(";")))


def precomp_stage(which, pre, d_i2, n1, n2, depth, w, ws, stream=None):
    """One stage of the precomputation on the multiply's workspace: STAGE_FWD_COLUMNS / _FWD_ROWS on
    operand 2, STAGE_PRE_STORE (B's row arrays -> pre)."""
    rc = lib().mpfft_precomp_stage(which, _ptr(pre), _nbytes(pre) if pre is not None else 0, _ptr(d_i2), n1, n2,
                                   depth, w, _ptr(ws), _nbytes(ws), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_precomp_stage({which})")


def mul_precomp_stage(which, d_i1, pre, d_r, n1, n2, depth, w, ws, stream=None):
    """One stage of the multiply on the workspace without B's arrays; STAGE_POINTWISE reads pre."""
    rc = lib().mpfft_mul_precomp_stage(which, _ptr(d_i1), _ptr(pre), _nbytes(pre) if pre is not None else 0,
                                       _ptr(d_r), n1, n2, depth, w, _ptr(ws), _nbytes(ws), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_mul_precomp_stage({which})")


class Precomp:
    """Host-pointer handle (mpfft_precomp_create): owns the device cache of operand `i2` for
    products with n1-limb operands at (depth, w), on the HIP device current at creation.  A context
    manager; close() frees the cache."""

    def __init__(self, i2, n1, depth, w):
        i2 = np.ascontiguousarray(i2, dtype=np.uint64)
        self.n1, self.n2, self.depth, self.w = n1, len(i2), depth, w
        h = _vp()
        rc = lib().mpfft_precomp_create(ctypes.byref(h), _p(i2), len(i2), n1, depth, w)
        if rc:
            raise MpfftError(rc, f"precomp_create(n1={n1}, n2={len(i2)}, depth={depth}, w={w})")
        self._h = h

    def close(self):
        if self._h is not None:
            lib().mpfft_precomp_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mul_precomp(i1, pre):
    """i1 * (the operand of the Precomp handle) as a new uint64 array of n1 + n2 limbs."""
    if pre._h is None:
        raise ValueError("the Precomp handle is closed")
    i1 = np.ascontiguousarray(i1, dtype=np.uint64)
    r = np.zeros(len(i1) + pre.n2, dtype=np.uint64)
    rc = lib().mpfft_mul_precomp_ex(_p(r), _p(i1), len(i1), pre._h)
    if rc:
        raise MpfftError(rc, f"mul_precomp(n1={len(i1)})")
    return r


# ---- products mod 2^B + 1, B = 64 L (mpfft_mulmod_*, include/mpfft.h): operands and result are
# L + 1 limbs, fully reduced (0 <= a <= 2^B) ----

def mulmod_check_params(L, depth, w):
    return lib().mpfft_mulmod_check_params(L, depth, w)


def mulmod(a, b, depth, w):
    """a b mod 2^(64 L) + 1 for L + 1-limb fully reduced a, b: a new uint64 array of L + 1 limbs."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if len(a) != len(b) or len(a) < 2:
        raise ValueError("operands are L + 1 limbs each")
    L = len(a) - 1
    r = np.zeros(L + 1, dtype=np.uint64)
    rc = lib().mpfft_mulmod_ex(_p(r), _p(a), _p(b), L, depth, w)
    if rc:
        raise MpfftError(rc, f"mulmod(L={L}, depth={depth}, w={w})")
    return r


def sqrmod(a, depth, w):
    """a^2 mod 2^(64 L) + 1 (one forward transform)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if len(a) < 2:
        raise ValueError("the operand is L + 1 limbs")
    L = len(a) - 1
    r = np.zeros(L + 1, dtype=np.uint64)
    rc = lib().mpfft_sqrmod_ex(_p(r), _p(a), L, depth, w)
    if rc:
        raise MpfftError(rc, f"sqrmod(L={L}, depth={depth}, w={w})")
    return r


def mulmod_workspace_bytes(L, depth, w, sqr=False):
    return int(lib().mpfft_mulmod_workspace_bytes(L, depth, w, int(bool(sqr))))


def alloc_workspace_mulmod(L, depth, w, sqr=False, device="cuda"):
    import torch
    nb = mulmod_workspace_bytes(L, depth, w, sqr)
    if nb == 0:
        raise MpfftError(mulmod_check_params(L, depth, w), "mulmod workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mulmod_device(d_r, d_a, d_b, L, depth, w, ws, stream=None):
    """d_r[:L+1] = d_a d_b mod 2^(64 L) + 1 on the GPU; queued on `stream`, not synchronised.
    d_r may not be an operand (it may be the next call's)."""
    rc = lib().mpfft_mulmod_device(_ptr(d_r), _ptr(d_a), _ptr(d_b), L, depth, w, _ptr(ws),
                                   ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mulmod_device")


def sqrmod_device(d_r, d_a, L, depth, w, ws, stream=None):
    rc = lib().mpfft_sqrmod_device(_ptr(d_r), _ptr(d_a), L, depth, w, _ptr(ws),
                                   ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_sqrmod_device")


def mulmod_plan_info(L, depth, w):
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_mulmod_plan_info(L, depth, w, out)
    if rc:
        raise MpfftError(rc, f"mulmod plan(L={L}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def mulmod_workspace_layout(L, depth, w, sqr=False):
    out = (ctypes.c_size_t * 8)()
    rc = lib().mpfft_mulmod_workspace_layout(L, depth, w, int(bool(sqr)), out)
    if rc:
        raise MpfftError(rc, "mulmod_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw")
    return dict(zip(keys, list(out)))


def mulmod_workspace_views(ws, L, depth, w, sqr=False):
    """(digA, topA, cbA) views into a mulmod workspace tensor (slot-major): limbs (slots, l) int64,
    carry limbs int32, carry masks (slots, cbw) int64."""
    import torch
    P = mulmod_plan_info(L, depth, w)
    lay = mulmod_workspace_layout(L, depth, w, sqr)
    slots, l, cbw = lay["slots"], P["l"], lay["cbw"]
    u8 = ws.view(torch.uint8)
    dig = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
    top = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
    cb = u8[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
    return dig, top, cb


def mulmod_stage(which, d_a, d_b, d_r, L, depth, w, ws, sqr=False, stream=None):
    rc = lib().mpfft_mulmod_stage(which, _ptr(d_a), _ptr(d_b), _ptr(d_r), L, depth, w, int(bool(sqr)), _ptr(ws),
                                  ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_mulmod_stage({which})")


def mulmod_stage_kernels(L, depth, w, sqr=False):
    """dict stage -> the kernel a product mod 2^(64 L) + 1 launches for it"""
    buf = ctypes.create_string_buffer(512)
    rc = lib().mpfft_mulmod_stage_kernels(L, depth, w, int(bool(sqr)), buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_mulmod_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


def mulmod_choose(L):
    """(depth, w) of least predicted time that are valid for this L."""
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmod_choose(L, ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmod_choose(L={L})")
    return int(d.value), int(w.value)


def mulmod_next_size(min_L):
    """(L, depth, w): an efficient modulus size L >= min_L and its parameters."""
    L, d, w = ctypes.c_long(), ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmod_next_size(min_L, ctypes.byref(L), ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmod_next_size({min_L})")
    return int(L.value), int(d.value), int(w.value)


# ---- products mod 2^B + 1 with the low-word CRT (mpfft_mulmodw_*, include/mpfft.h): the mulmod
# functions' mirrors, valid up to 2 bits1 + depth + 2 <= N + 32 (and from bits1 = 32 on) ----
STAGE_LOWCONV = 9   # mulmodw_stage: the low-word convolution d from the operands


def mulmodw_check_params(L, depth, w):
    return lib().mpfft_mulmodw_check_params(L, depth, w)


def mulmodw(a, b, depth, w):
    """a b mod 2^(64 L) + 1 for L + 1-limb fully reduced a, b: a new uint64 array of L + 1 limbs."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if len(a) != len(b) or len(a) < 2:
        raise ValueError("operands are L + 1 limbs each")
    L = len(a) - 1
    r = np.zeros(L + 1, dtype=np.uint64)
    rc = lib().mpfft_mulmodw_ex(_p(r), _p(a), _p(b), L, depth, w)
    if rc:
        raise MpfftError(rc, f"mulmodw(L={L}, depth={depth}, w={w})")
    return r


def sqrmodw(a, depth, w):
    """a^2 mod 2^(64 L) + 1 (one forward transform)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if len(a) < 2:
        raise ValueError("the operand is L + 1 limbs")
    L = len(a) - 1
    r = np.zeros(L + 1, dtype=np.uint64)
    rc = lib().mpfft_sqrmodw_ex(_p(r), _p(a), L, depth, w)
    if rc:
        raise MpfftError(rc, f"sqrmodw(L={L}, depth={depth}, w={w})")
    return r


def mulmodw_workspace_bytes(L, depth, w, sqr=False):
    return int(lib().mpfft_mulmodw_workspace_bytes(L, depth, w, int(bool(sqr))))


def alloc_workspace_mulmodw(L, depth, w, sqr=False, device="cuda"):
    import torch
    nb = mulmodw_workspace_bytes(L, depth, w, sqr)
    if nb == 0:
        raise MpfftError(mulmodw_check_params(L, depth, w), "mulmodw workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mulmodw_device(d_r, d_a, d_b, L, depth, w, ws, stream=None):
    """d_r[:L+1] = d_a d_b mod 2^(64 L) + 1 on the GPU; queued on `stream`, not synchronised.
    d_r may not be an operand (it may be the next call's)."""
    rc = lib().mpfft_mulmodw_device(_ptr(d_r), _ptr(d_a), _ptr(d_b), L, depth, w, _ptr(ws),
                                    ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodw_device")


def sqrmodw_device(d_r, d_a, L, depth, w, ws, stream=None):
    rc = lib().mpfft_sqrmodw_device(_ptr(d_r), _ptr(d_a), L, depth, w, _ptr(ws),
                                    ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_sqrmodw_device")


def mulmodw_plan_info(L, depth, w):
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_mulmodw_plan_info(L, depth, w, out)
    if rc:
        raise MpfftError(rc, f"mulmodw plan(L={L}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def mulmodw_workspace_layout(L, depth, w, sqr=False):
    out = (ctypes.c_size_t * 9)()
    rc = lib().mpfft_mulmodw_workspace_layout(L, depth, w, int(bool(sqr)), out)
    if rc:
        raise MpfftError(rc, "mulmodw_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw", "d")
    return dict(zip(keys, list(out)))


def mulmodw_workspace_views(ws, L, depth, w, sqr=False):
    """(digA, topA, cbA, d) views into a mulmodw workspace tensor (slot-major): limbs (slots, l) int64,
    carry limbs int32, carry masks (slots, cbw) int64, and the low-word convolution d, (slots,) int32
    (the words mod 2^32)."""
    import torch
    P = mulmodw_plan_info(L, depth, w)
    lay = mulmodw_workspace_layout(L, depth, w, sqr)
    slots, l, cbw = lay["slots"], P["l"], lay["cbw"]
    u8 = ws.view(torch.uint8)
    dig = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
    top = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
    cb = u8[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
    d = u8[lay["d"]:lay["d"] + slots * 4].view(torch.int32)
    return dig, top, cb, d


def mulmodw_stage(which, d_a, d_b, d_r, L, depth, w, ws, sqr=False, stream=None):
    rc = lib().mpfft_mulmodw_stage(which, _ptr(d_a), _ptr(d_b), _ptr(d_r), L, depth, w, int(bool(sqr)), _ptr(ws),
                                   ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_mulmodw_stage({which})")


def mulmodw_stage_kernels(L, depth, w, sqr=False):
    """dict stage -> the kernel a product mod 2^(64 L) + 1 launches for it"""
    buf = ctypes.create_string_buffer(512)
    rc = lib().mpfft_mulmodw_stage_kernels(L, depth, w, int(bool(sqr)), buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodw_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


def mulmodw_choose(L):
    """(depth, w) of least predicted time that are valid for this L."""
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmodw_choose(L, ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmodw_choose(L={L})")
    return int(d.value), int(w.value)


def mulmodw_next_size(min_L):
    """(L, depth, w): an efficient modulus size L >= min_L and its parameters."""
    L, d, w = ctypes.c_long(), ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmodw_next_size(min_L, ctypes.byref(L), ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmodw_next_size({min_L})")
    return int(L.value), int(d.value), int(w.value)


# ---- products mod 2^B - 1, B = 64 L (mpfft_mulmodm1_*, include/mpfft.h): operands and result are
# L limbs; any operand value is valid, the result is fully reduced (never all-ones) ----
M1_MUL, M1_SQR, M1_PRE = 0, 1, 2   # plan kinds: multiply, square, multiply against a cached operand


def mulmodm1_check_params(L, depth, w):
    return lib().mpfft_mulmodm1_check_params(L, depth, w)


def mulmodm1(a, b, depth, w):
    """a b mod 2^(64 L) - 1 for L-limb a, b: a new uint64 array of L limbs, fully reduced."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if len(a) != len(b) or len(a) < 1:
        raise ValueError("operands are L limbs each")
    L = len(a)
    r = np.zeros(L, dtype=np.uint64)
    rc = lib().mpfft_mulmodm1_ex(_p(r), _p(a), _p(b), L, depth, w)
    if rc:
        raise MpfftError(rc, f"mulmodm1(L={L}, depth={depth}, w={w})")
    return r


def sqrmodm1(a, depth, w):
    """a^2 mod 2^(64 L) - 1 (one forward transform)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if len(a) < 1:
        raise ValueError("the operand is L limbs")
    L = len(a)
    r = np.zeros(L, dtype=np.uint64)
    rc = lib().mpfft_sqrmodm1_ex(_p(r), _p(a), L, depth, w)
    if rc:
        raise MpfftError(rc, f"sqrmodm1(L={L}, depth={depth}, w={w})")
    return r


def mulmodm1_workspace_bytes(L, depth, w, kind=M1_MUL):
    return int(lib().mpfft_mulmodm1_workspace_bytes(L, depth, w, int(kind)))


def alloc_workspace_mulmodm1(L, depth, w, kind=M1_MUL, device="cuda"):
    import torch
    nb = mulmodm1_workspace_bytes(L, depth, w, kind)
    if nb == 0:
        raise MpfftError(mulmodm1_check_params(L, depth, w) or 1, "mulmodm1 workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mulmodm1_device(d_r, d_a, d_b, L, depth, w, ws, stream=None):
    """d_r[:L] = d_a d_b mod 2^(64 L) - 1 on the GPU; queued on `stream`, not synchronised.
    d_r may not overlap an operand (it may be the next call's)."""
    rc = lib().mpfft_mulmodm1_device(_ptr(d_r), _ptr(d_a), _ptr(d_b), L, depth, w, _ptr(ws),
                                     ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodm1_device")


def sqrmodm1_device(d_r, d_a, L, depth, w, ws, stream=None):
    rc = lib().mpfft_sqrmodm1_device(_ptr(d_r), _ptr(d_a), L, depth, w, _ptr(ws),
                                     ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_sqrmodm1_device")


def mulmodm1_plan_info(L, depth, w):
    out = (ctypes.c_long * 10)()
    rc = lib().mpfft_mulmodm1_plan_info(L, depth, w, out)
    if rc:
        raise MpfftError(rc, f"mulmodm1 plan(L={L}, depth={depth}, w={w})")
    keys = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
    return dict(zip(keys, list(out)))


def mulmodm1_workspace_layout(L, depth, w, kind=M1_MUL):
    out = (ctypes.c_size_t * 8)()
    rc = lib().mpfft_mulmodm1_workspace_layout(L, depth, w, int(kind), out)
    if rc:
        raise MpfftError(rc, "mulmodm1_workspace_layout")
    keys = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw")
    return dict(zip(keys, list(out)))


def mulmodm1_workspace_views(ws, L, depth, w, kind=M1_MUL):
    """(digA, topA, cbA) views into a mulmodm1 workspace tensor (slot-major): limbs (slots, l) int64,
    carry limbs int32, carry masks (slots, cbw) int64."""
    import torch
    P = mulmodm1_plan_info(L, depth, w)
    lay = mulmodm1_workspace_layout(L, depth, w, kind)
    slots, l, cbw = lay["slots"], P["l"], lay["cbw"]
    u8 = ws.view(torch.uint8)
    dig = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
    top = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
    cb = u8[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
    return dig, top, cb


def mulmodm1_stage(which, d_a, d_b, d_r, L, depth, w, ws, kind=M1_MUL, stream=None):
    rc = lib().mpfft_mulmodm1_stage(which, _ptr(d_a), _ptr(d_b), _ptr(d_r), L, depth, w, int(kind), _ptr(ws),
                                    ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_mulmodm1_stage({which})")


def mulmodm1_stage_kernels(L, depth, w, kind=M1_MUL):
    """dict stage -> the kernel a product mod 2^(64 L) - 1 launches for it"""
    buf = ctypes.create_string_buffer(512)
    rc = lib().mpfft_mulmodm1_stage_kernels(L, depth, w, int(kind), buf, len(buf))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodm1_stage_kernels")
    return dict(zip(STAGE_NAMES, buf.value.decode().split(";")))


def mulmodm1_choose(L):
    """(depth, w) of least predicted time that are valid for this L."""
    d, w = ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmodm1_choose(L, ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmodm1_choose(L={L})")
    return int(d.value), int(w.value)


def mulmodm1_next_size(min_L):
    """(L, depth, w): an efficient modulus size L >= min_L and its parameters."""
    L, d, w = ctypes.c_long(), ctypes.c_ulong(), ctypes.c_ulong()
    rc = lib().mpfft_mulmodm1_next_size(min_L, ctypes.byref(L), ctypes.byref(d), ctypes.byref(w))
    if rc:
        raise MpfftError(rc, f"mulmodm1_next_size({min_L})")
    return int(L.value), int(d.value), int(w.value)


def mulmodm1_precomp_bytes(L, depth, w):
    return int(lib().mpfft_mulmodm1_precomp_bytes(L, depth, w))


def alloc_precomp_mulmodm1(L, depth, w, device="cuda"):
    import torch
    nb = mulmodm1_precomp_bytes(L, depth, w)
    if nb == 0:
        raise MpfftError(mulmodm1_check_params(L, depth, w) or 1, "mulmodm1 precomp")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def mulmodm1_precomp_device(pre, d_b, L, depth, w, ws, stream=None):
    """The cache of operand d_b (L limbs) for products mod 2^(64 L) - 1 against it; ws: the
    multiply's workspace (kind M1_MUL)."""
    rc = lib().mpfft_mulmodm1_precomp_device(_ptr(pre), pre.numel() * pre.element_size(), _ptr(d_b), L, depth, w,
                                             _ptr(ws), ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodm1_precomp_device")


def mulmodm1_mul_precomp_device(d_r, d_a, pre, L, depth, w, ws, stream=None):
    """d_r[:L] = d_a (the cached operand) mod 2^(64 L) - 1; ws: the workspace of kind M1_PRE; pre is
    only read."""
    rc = lib().mpfft_mulmodm1_mul_precomp_device(_ptr(d_r), _ptr(d_a), _ptr(pre), pre.numel() * pre.element_size(), L,
                                                 depth, w, _ptr(ws), ws.numel() * ws.element_size(), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_mulmodm1_mul_precomp_device")


# ---- sharded (multi-GPU) stages: see sharded.py ------------------------------

def shard_desc(sh):
    """dict from sharded.ShardedMul.shard_desc() -> struct mpfft_shard"""
    d = _Shard()
    for k in ("n1", "n2", "depth", "w", "c0", "ccount", "r0", "rcount", "ccb"):
        setattr(d, k, int(sh[k]))
    for k in (0, 1):
        d.col_dig[k] = sh["col"][k]["dig"].data_ptr()
        d.col_cb[k] = sh["col"][k]["cb"].data_ptr()
        d.col_top[k] = sh["col"][k]["top"].data_ptr()
        d.row_dig[k] = sh["row"][k]["dig"].data_ptr()
        d.row_cb[k] = sh["row"][k]["cb"].data_ptr()
        d.row_top[k] = sh["row"][k]["top"].data_ptr()
    d.src_chunk = int(sh.get("src_chunk", 0))
    rc = sh.get("rowc")
    if rc is not None:
        d.rowc_dig, d.rowc_cb, d.rowc_top = rc["dig"].data_ptr(), rc["cb"].data_ptr(), rc["top"].data_ptr()
    return d


def shard_row_fused(n1, n2, depth, w, ccb):
    """True if the sharded row stages fuse the last row DIF level into the pointwise
    (the caller then supplies a third row-layout array, `rowc`)."""
    return bool(lib().mpfft_shard_row_fused(n1, n2, depth, w, ccb))


def shard_stage(which, desc, d_i1, d_i2, stream=None):
    rc = lib().mpfft_shard_stage(which, ctypes.byref(desc), _ptr(d_i1), _ptr(d_i2), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_shard_stage({which})")


def shard_stage_rows(which, desc, lo, hi, stream=None):
    """The row stages (SHARD_FWD_ROWS / POINTWISE / INV_ROWS) on local rows [lo, hi) only."""
    rc = lib().mpfft_shard_stage_rows(which, ctypes.byref(desc), lo, hi, _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_shard_stage_rows({which}, {lo}, {hi})")


def shard_combine_tmp_bytes(n1, n2, depth, w, world):
    return int(lib().mpfft_shard_combine_tmp_bytes(n1, n2, depth, w, world))


def shard_combine(desc, phase, d_r, halo, d_sums, d_sums_all, tmp, stream=None):
    """The rank's product stripes from its column layout (include/mpfft.h mpfft_shard_combine):
    phase 0 with carry-in 0 + stripe summaries into d_sums, phase 1 the carries from d_sums_all."""
    rc = lib().mpfft_shard_combine(ctypes.byref(desc), phase, _ptr(d_r), _ptr(halo), _ptr(d_sums), _ptr(d_sums_all),
                                   _ptr(tmp), tmp.numel(), _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_shard_combine(phase {phase})")


# ---- multi-GPU from one process (mpfft_mul_multi, multi.hip) ------------------------

def shard_partition(n1, n2, depth, w, world):
    """The C partition of one column-sharded multiply: dict rows (list of world + 1), C, chunk,
    H, Tr, fused, SL, S, ms (the stripes' first product limbs, S + 1) (mpfft_shard_partition,
    mpfft_shard_stripes)."""
    rows = (ctypes.c_long * (world + 1))()
    info = (ctypes.c_long * 7)()
    rc = lib().mpfft_shard_partition(n1, n2, depth, w, world, rows, info)
    if rc:
        raise MpfftError(rc, f"shard_partition(world={world})")
    S = info[6]
    ms = (ctypes.c_long * (S + 1))()
    n = lib().mpfft_shard_stripes(n1, n2, depth, w, world, ms, S + 1)
    if n != S + 1:
        raise MpfftError(-n if n < 0 else 1, "shard_stripes")
    return {"rows": list(rows), "C": info[0], "chunk": info[1], "H": info[2], "Tr": info[3],
            "fused": bool(info[4]), "SL": info[5], "S": S, "ms": list(ms)}


def _copies(fn, *args):
    n = fn(*args, None, 0)
    if n < 0:
        raise MpfftError(-n, fn.__name__)
    out = (_Copy * max(n, 1))()
    n = fn(*args, out, n)
    if n < 0:
        raise MpfftError(-n, fn.__name__)
    return [{f: getattr(out[i], f) for f, _ in _Copy._fields_} for i in range(n)]


def shard_exchange_plan(n1, n2, depth, w, world, which):
    """The copies of exchange `which` (XCHG_*): list of dicts (mpfft_shard_exchange_plan)."""
    return _copies(lib().mpfft_shard_exchange_plan, n1, n2, depth, w, world, which)


def shard_halo_plan(n1, n2, depth, w, world):
    """The halo copies before the combine (mpfft_shard_halo_plan): column layout -> halo, limbs."""
    return _copies(lib().mpfft_shard_halo_plan, n1, n2, depth, w, world)


def shard_src_limbs(n1, n2, depth, w, world):
    n = lib().mpfft_shard_src_limbs(n1, n2, depth, w, world)
    if n < 0:
        raise MpfftError(-n, "shard_src_limbs")
    return n


def shard_pack(a, n1, n2, depth, w, world, rank):
    """rank's operand slices of operand `a` (uint64 limbs), as the device-resident multi-GPU
    entry and the sharded drivers read them (mpfft_shard_pack)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    out = np.empty(shard_src_limbs(n1, n2, depth, w, world), dtype=np.uint64)
    rc = lib().mpfft_shard_pack(n1, n2, depth, w, world, rank, _p(a), len(a), _p(out))
    if rc:
        raise MpfftError(rc, "shard_pack")
    return out


def mul_multi_device(n1, n2, depth, w, devices, src1, src2, outs, streams=None):
    """Device-resident multi-GPU multiply (mpfft_mul_multi_device): src1[g], src2[g] rank g's
    packed slices on devices[g] (torch tensors), outs[g] its Tr * SL stripe limbs.  streams:
    torch streams per rank (the work is ordered on them), or None (returns when done)."""
    G = len(devices)
    devs = (ctypes.c_int * G)(*devices)
    P = (_vp * G)
    s1 = P(*[t.data_ptr() for t in src1])
    s2 = P(*[t.data_ptr() for t in src2])
    r = P(*[t.data_ptr() for t in outs])
    st = P(*[s.cuda_stream for s in streams]) if streams is not None else None
    rc = lib().mpfft_mul_multi_device(n1, n2, depth, w, G, devs, s1, s2, r, st)
    if rc:
        raise MpfftError(rc, f"mul_multi_device(devices={list(devices)})")


def assemble_stripes(part, world, stripes):
    """The product from every rank's stripe buffers (stripes[g]: Tr * SL limbs, uint64)."""
    ms, SL = part["ms"], part["SL"]
    out = np.empty(ms[-1], dtype=np.uint64)
    for s in range(len(ms) - 1):
        g, j = s % world, s // world
        n = ms[s + 1] - ms[s]
        out[ms[s]: ms[s + 1]] = stripes[g][j * SL: j * SL + n]
    return out


def mul_multi(i1, i2, depth, w, devices):
    """r = i1 * i2 column-sharded over len(devices) ranks (devices may repeat), one process."""
    i1 = np.ascontiguousarray(i1, dtype=np.uint64)
    i2 = np.ascontiguousarray(i2, dtype=np.uint64)
    r = np.zeros(len(i1) + len(i2), dtype=np.uint64)
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib().mpfft_mul_multi(_p(r), _p(i1), len(i1), _p(i2), len(i2), depth, w, len(devices), devs)
    if rc:
        raise MpfftError(rc, f"mul_multi(devices={list(devices)})")
    return r


def set_devices(devices, min_l=0):
    """new_mpn_mul policy: shard products with >= min_l-limb coefficients over `devices`."""
    devs = (ctypes.c_int * max(len(devices), 1))(*devices)
    return lib().mpfft_set_devices(len(devices), devs, min_l)


def multi_release():
    return lib().mpfft_multi_release()


def multi_schedule(n1, n2, depth, w, world, calls=1):
    """The event graph of `calls` back-to-back device-resident multi-rank multiplies
    (mpfft_multi_schedule: a dry run, no GPU): list of (kind, rank, stream, *rest) tuples."""
    n = lib().mpfft_multi_schedule(n1, n2, depth, w, world, calls, None, 0)
    if n < 0:
        raise MpfftError(-n, "multi_schedule")
    buf = ctypes.create_string_buffer(n)
    lib().mpfft_multi_schedule(n1, n2, depth, w, world, calls, buf, n)
    out = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        out.append(tuple([f[0]] + [int(x) if x.lstrip("-").isdigit() else x for x in f[1:]]))
    return out
