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


_I, _SZ, _U64, _cp = ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_char_p
_ip, _lp, _ulp, _szp, _pp = (ctypes.POINTER(t) for t in (_I, _L, _UL, _SZ, _vp))
_MUL = [_L, _L, _UL, _UL]    # (n1, n2, depth, w)
_MOD = [_L, _UL, _UL]        # (L, depth, w), and a square's (n, depth, w)
_DOT = [_L] + _MUL           # (K, n1, n2, depth, w)
_MM = [_L, _L, _L] + _MUL    # (m, k, p, n1, n2, depth, w)
_WS = [_vp, _SZ, _vp]        # (d_ws, ws_bytes, stream)
_TEXT = [_cp, _SZ]           # (buf, len)


def _mod_signatures(fam, sq):
    """the entries every family of products modulo 2^B +- 1 has: mpfft_<fam>_* and the squares' mpfft_<sq>_*"""
    return [("mpfft_%s_check_params" % fam, _I, _MOD), ("mpfft_%s_ex" % fam, _I, [_u64p, _u64p, _u64p] + _MOD),
            ("mpfft_%s_ex" % sq, _I, [_u64p, _u64p] + _MOD), ("mpfft_%s_device" % fam, _I, [_vp, _vp, _vp] + _MOD + _WS),
            ("mpfft_%s_device" % sq, _I, [_vp, _vp] + _MOD + _WS), ("mpfft_%s_workspace_bytes" % fam, _SZ, _MOD + [_I]),
            ("mpfft_%s_plan_info" % fam, _I, _MOD + [_lp]), ("mpfft_%s_workspace_layout" % fam, _I, _MOD + [_I, _szp]),
            ("mpfft_%s_stage" % fam, _I, [_I, _vp, _vp, _vp] + _MOD + [_I] + _WS),
            ("mpfft_%s_stage_kernels" % fam, _I, _MOD + [_I] + _TEXT), ("mpfft_%s_choose" % fam, _I, [_L, _ulp, _ulp]),
            ("mpfft_%s_next_size" % fam, _I, [_L, _lp, _ulp, _ulp])]


def _signatures():
    """(name, restype, argtypes) of every function of include/mpfft.h that is called from here: a wrong entry
    corrupts arguments silently, so tests/test_signature_table.py holds each against the header's prototype"""
    return [
        ("new_mpn_mul", None, [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]),
        ("mpfft_mul_ex", _I, [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]),
        ("mpfft_profile_begin", _I, [_I]), ("mpfft_profile_end", _I, [ctypes.POINTER(ctypes.c_float), _ip]),
        ("mpfft_stage_kernels", _I, _MUL + _TEXT), ("mpfft_inv_columns_schedule", _I, _MUL + _TEXT),
        ("mpfft_release", _I, []),
        ("mpfft_mul_device", _I, [_vp, _vp, _L, _vp, _L, _UL, _UL] + _WS),
        ("mpfft_stage", _I, [_I, _vp, _vp, _vp] + _MUL + _WS),
        ("mpfft_workspace_bytes", _SZ, _MUL), ("mpfft_check_params", _I, _MUL), ("mpfft_plan_info", _I, _MUL + [_lp]),
        ("mpfft_workspace_layout", _I, _MUL + [_szp]),
        ("mpfft_strerror", _cp, [_I]), ("mpfft_version", _I, []), ("mpfft_fill_random", None, [_u64p, _L, _U64]),
        ("mpfft_shard_stage", _I, [_I, ctypes.POINTER(_Shard), _vp, _vp, _vp]),
        ("mpfft_shard_stage_rows", _I, [_I, ctypes.POINTER(_Shard), _I, _I, _vp]),
        ("mpfft_shard_row_fused", _I, _MUL + [_I]), ("mpfft_shard_combine_tmp_bytes", _SZ, _MUL + [_I]),
        ("mpfft_shard_combine", _I, [ctypes.POINTER(_Shard), _I, _vp, _vp, _vp, _vp, _vp, _SZ, _vp]),
        ("mpfft_shard_partition", _I, _MUL + [_I, _lp, _lp]), ("mpfft_shard_stripes", _L, _MUL + [_I, _lp, _L]),
        ("mpfft_shard_exchange_plan", _L, _MUL + [_I, _I, ctypes.POINTER(_Copy), _L]),
        ("mpfft_shard_halo_plan", _L, _MUL + [_I, ctypes.POINTER(_Copy), _L]),
        ("mpfft_shard_src_limbs", _L, _MUL + [_I]), ("mpfft_shard_pack", _I, _MUL + [_I, _I, _u64p, _L, _u64p]),
        ("mpfft_mul_multi_device", _I, _MUL + [_I, _ip, _pp, _pp, _pp, _pp]),
        ("mpfft_mul_multi", _I, [_u64p, _u64p, _L, _u64p, _L, _UL, _UL, _I, _ip]),
        ("mpfft_multi_release", _I, []), ("mpfft_multi_schedule", _L, _MUL + [_I, _I] + _TEXT),
        ("mpfft_set_devices", _I, [_I, _ip, _L]), ("mpfft_last_ngpus", _I, []),
        ("mpfft_choose", _I, [_L, _L, _ulp, _ulp]), ("mpfft_mul_auto", _I, [_u64p, _u64p, _L, _u64p, _L]),
        ("new_mpn_mul6", None, [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]),
        ("mpfft_mul6_ex", _I, [_u64p, _u64p, _L, _u64p, _L, _UL, _UL]),
        ("mpfft_mul6_device", _I, [_vp, _vp, _L, _vp, _L, _UL, _UL] + _WS),
        ("mpfft_workspace_bytes6", _SZ, _MUL), ("mpfft_check_params6", _I, _MUL), ("mpfft_plan_info6", _I, _MUL + [_lp]),
        # MPFFT_VERSION 3: squares
        ("mpfft_sqr_ex", _I, [_u64p, _u64p] + _MOD), ("mpfft_sqr_auto", _I, [_u64p, _u64p, _L]),
        ("mpfft_sqr_device", _I, [_vp, _vp] + _MOD + _WS), ("mpfft_sqr_workspace_bytes", _SZ, _MOD),
        ("mpfft_sqr_workspace_layout", _I, _MOD + [_szp]), ("mpfft_sqr_stage", _I, [_I, _vp, _vp] + _MOD + _WS),
        ("mpfft_sqr_stage_kernels", _I, _MOD + _TEXT),
        # 5: the cached operand
        ("mpfft_precomp_bytes", _SZ, _MUL), ("mpfft_precomp_device", _I, [_vp, _SZ, _vp] + _MUL + _WS),
        ("mpfft_mul_precomp_workspace_bytes", _SZ, _MUL),
        ("mpfft_mul_precomp_device", _I, [_vp, _vp, _L, _vp, _SZ, _L, _UL, _UL] + _WS),
        ("mpfft_precomp_stage_kernels", _I, _MUL + _TEXT), ("mpfft_precomp_stage", _I, [_I, _vp, _SZ, _vp] + _MUL + _WS),
        ("mpfft_mul_precomp_stage", _I, [_I, _vp, _vp, _SZ, _vp] + _MUL + _WS),
        ("mpfft_precomp_create", _I, [_pp, _u64p, _L, _L, _UL, _UL]), ("mpfft_mul_precomp_ex", _I, [_u64p, _u64p, _L, _vp]),
        ("mpfft_precomp_destroy", None, [_vp]),
        # 6: mod 2^B - 1 and its cached operand
        ("mpfft_mulmodm1_precomp_bytes", _SZ, _MOD), ("mpfft_mulmodm1_precomp_device", _I, [_vp, _SZ, _vp] + _MOD + _WS),
        ("mpfft_mulmodm1_mul_precomp_device", _I, [_vp, _vp, _vp, _SZ] + _MOD + _WS),
        # 8: sums of products
        ("mpfft_dot_check_params", _I, _DOT), ("mpfft_dot_plan_info", _I, _DOT + [_lp]),
        ("mpfft_dot_choose", _I, [_L, _L, _L, _ulp, _ulp]), ("mpfft_dot_workspace_bytes", _SZ, _DOT),
        ("mpfft_dot_workspace_layout", _I, _DOT + [_szp]), ("mpfft_dot_device", _I, [_vp, _L, _pp, _pp] + _MUL + _WS),
        ("mpfft_dot_ex", _I, [_u64p, _L, _pp, _pp] + _MUL), ("mpfft_dot_auto", _I, [_u64p, _L, _pp, _pp, _L, _L]),
        ("mpfft_dot_stage_kernels", _I, _DOT + _TEXT), ("mpfft_dot_stage", _I, [_I, _L, _vp, _vp, _vp] + _MUL + _WS),
        # 9: signed sums
        ("mpfft_sdot_check_params", _I, [_L, _U64] + _MUL), ("mpfft_sdot_workspace_bytes", _SZ, _DOT),
        ("mpfft_sdot_workspace_layout", _I, _DOT + [_szp]),
        ("mpfft_sdot_device", _I, [_vp, _L, _U64, _pp, _pp] + _MUL + _WS),
        ("mpfft_sdot_ex", _I, [_u64p, _L, _U64, _pp, _pp] + _MUL), ("mpfft_sdot_auto", _I, [_u64p, _L, _U64, _pp, _pp, _L, _L]),
        ("mpfft_sdot_stage_kernels", _I, [_L, _U64] + _MUL + _TEXT),
        ("mpfft_sdot_stage", _I, [_I, _L, _vp, _vp, _vp] + _MUL + _WS),
        # 10: small matrix products
        ("mpfft_matmul_check_params", _I, _MM), ("mpfft_matmul_workspace_bytes", _SZ, _MM),
        ("mpfft_matmul_workspace_layout", _I, _MM + [_szp]),
        ("mpfft_matmul_device", _I, [_pp, _L, _L, _L, _pp, _pp] + _MUL + _WS),
        ("mpfft_matmul_ex", _I, [_pp, _L, _L, _L, _pp, _pp] + _MUL), ("mpfft_matmul_auto", _I, [_pp, _L, _L, _L, _pp, _pp, _L, _L]),
        ("mpfft_matmul_stage_kernels", _I, _MM + _TEXT),
        ("mpfft_matmul_stage", _I, [_I, _L, _L, _L, _vp, _vp, _vp] + _MUL + _WS + [_L, _ip, _ip]),
        # 4, 7, 6: mod 2^B + 1, with the low-word CRT, mod 2^B - 1
    ] + _mod_signatures("mulmod", "sqrmod") + _mod_signatures("mulmodw", "sqrmodw") + _mod_signatures("mulmodm1", "sqrmodm1")


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
        for name, restype, argtypes in _signatures():
            f = getattr(h, name, None)
            if f is None:   # (older libraries in A/B runs through MPFFT_LIB lack the later versions' entries)
                continue
            f.restype, f.argtypes = restype, argtypes
        _lib = h
    return _lib


def strerror(code):
    return lib().mpfft_strerror(int(code)).decode()


def _p(a):
    if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("limb arrays must be C-contiguous numpy.uint64")
    return a.ctypes.data_as(_u64p)


_PLAN_KEYS = ("n", "l", "NC", "j1", "j2", "trunc", "bits1", "NR", "tpb", "U")
_LAYOUT_KEYS = ("digA", "topA", "cbA", "digB", "topB", "cbB", "slots", "cbw")


def _plan_info(fn, what, *args):
    """a *_plan_info entry's ten words as a dict, or MpfftError(what)"""
    out = (ctypes.c_long * len(_PLAN_KEYS))()
    rc = fn(*args, out)
    if rc:
        raise MpfftError(rc, what)
    return dict(zip(_PLAN_KEYS, list(out)))


def _layout(fn, what, keys, *args):
    """a *_workspace_layout entry's words as a dict under `keys`"""
    out = (ctypes.c_size_t * len(keys))()
    rc = fn(*args, out)
    if rc:
        raise MpfftError(rc, what)
    return dict(zip(keys, list(out)))


def _kernel_names(fn, what, size, fields, *args):
    """a *_stage_kernels entry's ';'-joined text (at most size bytes) as a dict under `fields`"""
    buf = ctypes.create_string_buffer(size)
    rc = fn(*args, buf, len(buf))
    if rc:
        raise MpfftError(rc, what)
    return dict(zip(fields, buf.value.decode().split(";")))


def check_params(n1, n2, depth, w):
    return lib().mpfft_check_params(n1, n2, depth, w)


def plan_info(n1, n2, depth, w):
    """dict of the derived parameters (mul_fft.c:3193-3203) or MpfftError."""
    return _plan_info(lib().mpfft_plan_info, f"plan(n1={n1}, n2={n2}, depth={depth}, w={w})", n1, n2, depth, w)


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
    return _plan_info(lib().mpfft_plan_info6, f"plan6(n1={n1}, n2={n2}, depth={depth}, w={w})", n1, n2, depth, w)


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
    return _kernel_names(lib().mpfft_stage_kernels, "mpfft_stage_kernels", 512, STAGE_NAMES, n1, n2, depth, w)


def inv_columns_schedule(n1, n2, depth, w):
    """The launches of the single-device truncated inverse column transform, in order (a host-side
    dry run: needs no GPU)."""
    buf = ctypes.create_string_buffer(1 << 16)
    rc = lib().mpfft_inv_columns_schedule(n1, n2, depth, w, buf, len(buf))
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
    return _layout(lib().mpfft_workspace_layout, "workspace_layout", _LAYOUT_KEYS, n1, n2, depth, w)


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
    return _kernel_names(lib().mpfft_sqr_stage_kernels, "mpfft_sqr_stage_kernels", 512, STAGE_NAMES, n, depth, w)


def sqr_workspace_layout(n, depth, w):
    return _layout(lib().mpfft_sqr_workspace_layout, "sqr_workspace_layout", _LAYOUT_KEYS, n, depth, w)


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
# pairs and one inverse; the workspace has a third coefficient array C, the accumulator.
# Signed sums (mpfft_sdot_*): r = sum_i +-a_i b_i on the dot plan (dot_choose, dot_plan_info,
# dot_max_limbs); the workspace is the dot's followed by the complement scratch and the accumulator D
# of the subtracted b_i.  The sdot_* wrappers are the dot_* ones with the sign mask `neg` passed on. ----

DOT_MAX = 64
STAGE_ACC = 0x200   # dot_stage: or-ed onto STAGE_POINTWISE, C <- C + A B
STAGE_SD_NEG = 10   # sdot_stage: d_a -> complement scratch, D <- d_b (| STAGE_ACC: D <- D + d_b)
STAGE_SD_FIX = 11   # sdot_stage: d_r <- d_r + D - (D << 64 n1)
SDOT_FIX_BLOCK = 4096   # limbs per block of the correction's carry chain (MPFFT_SDOT_FIX_BLOCK)
_DOT_LAYOUT_KEYS = _LAYOUT_KEYS + ("digC", "topC", "cbC")


def _neg_mask(neg):
    """the sign mask as an int: an int is taken as it is, a sequence of booleans gives bit i = neg[i]"""
    if isinstance(neg, (int, np.integer)) and not isinstance(neg, (bool, np.bool_)):
        neg = int(neg)
    else:
        neg = sum(1 << i for i, x in enumerate(neg) if x)
    if neg < 0 or neg >> 64:
        raise ValueError("neg is a 64-bit mask")
    return neg


def _dot_entry(entry, neg):
    """(the name, mpfft_dot_<entry> or with a mask mpfft_sdot_<entry>; that function; the mask argument, if any)"""
    name = "%s_%s" % ("dot" if neg is None else "sdot", entry)
    return name, getattr(lib(), "mpfft_" + name), () if neg is None else (_neg_mask(neg),)


def sdot_to_int(limbs):
    """the signed Python integer of a two's-complement little-endian limb array"""
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
    v = int.from_bytes(limbs.tobytes(), "little")
    return v - (1 << (64 * len(limbs))) if len(limbs) and int(limbs[-1]) >> 63 else v


def dot_check_params(K, n1, n2, depth, w):
    return lib().mpfft_dot_check_params(K, n1, n2, depth, w)


def sdot_check_params(K, neg, n1, n2, depth, w):
    return lib().mpfft_sdot_check_params(K, _neg_mask(neg), n1, n2, depth, w)


def dot_plan_info(K, n1, n2, depth, w):
    """plan_info of a K-term sum: bits1 = (N - depth - ceil(log2 K)) / 2 and what follows from it"""
    return _plan_info(lib().mpfft_dot_plan_info, f"dot plan(K={K}, n1={n1}, n2={n2}, depth={depth}, w={w})",
                      K, n1, n2, depth, w)


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


def sdot_workspace_bytes(K, n1, n2, depth, w):
    return int(lib().mpfft_sdot_workspace_bytes(K, n1, n2, depth, w))


def _alloc_workspace_dot(nb, what, K, n1, n2, depth, w, device):
    import torch
    if nb == 0:
        raise MpfftError(dot_check_params(K, n1, n2, depth, w), what)
    return torch.empty(nb, dtype=torch.uint8, device=device)


def alloc_workspace_dot(K, n1, n2, depth, w, device="cuda"):
    return _alloc_workspace_dot(dot_workspace_bytes(K, n1, n2, depth, w), "dot workspace", K, n1, n2, depth, w, device)


def alloc_workspace_sdot(K, n1, n2, depth, w, device="cuda"):
    return _alloc_workspace_dot(sdot_workspace_bytes(K, n1, n2, depth, w), "sdot workspace", K, n1, n2, depth, w, device)


def dot_workspace_layout(K, n1, n2, depth, w):
    return _layout(lib().mpfft_dot_workspace_layout, "dot_workspace_layout", _DOT_LAYOUT_KEYS, K, n1, n2, depth, w)


def sdot_workspace_layout(K, n1, n2, depth, w):
    """dot_workspace_layout's entries, then "scratch" (the complement, n1 limbs) and "D" (n2 limbs)"""
    return _layout(lib().mpfft_sdot_workspace_layout, "sdot_workspace_layout", _DOT_LAYOUT_KEYS + ("scratch", "D"),
                   K, n1, n2, depth, w)


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


def _dot_device(neg, d_r, d_as, d_bs, n1, n2, depth, w, ws, stream):
    if len(d_as) != len(d_bs):
        raise ValueError("as many a_i as b_i")
    name, fn, mask = _dot_entry("device", neg)
    rc = fn(_ptr(d_r), len(d_as), *mask, _ptr_array(d_as), _ptr_array(d_bs), n1, n2, depth, w, _ptr(ws), _nbytes(ws),
            _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_" + name)


def dot_device(d_r, d_as, d_bs, n1, n2, depth, w, ws, stream=None):
    """d_r[:n1 + n2 + 1] = sum_i d_as[i][:n1] * d_bs[i][:n2], all tensors on the GPU (lists of K
    tensors; the same tensor may appear more than once); queued on `stream`, not synchronised."""
    _dot_device(None, d_r, d_as, d_bs, n1, n2, depth, w, ws, stream)


def sdot_device(d_r, d_as, d_bs, neg, n1, n2, depth, w, ws, stream=None):
    """d_r[:n1 + n2 + 1] = sum_i +-d_as[i][:n1] * d_bs[i][:n2] in two's complement, term i subtracted
    where neg (an int mask or a sequence of booleans) says so; as dot_device otherwise."""
    _dot_device(neg, d_r, d_as, d_bs, n1, n2, depth, w, ws, stream)


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


def _dot(neg, a_list, b_list, depth, w):
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    name, fn, mask = _dot_entry("ex", neg)
    rc = fn(_p(r), len(a_list), *mask, pa, pb, n1, n2, depth, w)
    if rc:
        raise MpfftError(rc, f"{name[:-3]}(K={len(a_list)}, n1={n1}, n2={n2}, depth={depth}, w={w})")
    return r


def dot(a_list, b_list, depth, w):
    """sum_i a_list[i] * b_list[i] as a new uint64 array of n1 + n2 + 1 limbs (host pointers, mpfft_dot_ex)"""
    return _dot(None, a_list, b_list, depth, w)


def sdot(a_list, b_list, neg, depth, w):
    """sum_i +-a_list[i] * b_list[i] as a new uint64 array of n1 + n2 + 1 limbs, two's complement
    (host pointers, mpfft_sdot_ex); sdot_to_int gives its signed value"""
    return _dot(neg, a_list, b_list, depth, w)


def _dot_auto(neg, a_list, b_list):
    a_list, b_list, pa, pb, n1, n2 = _host_terms(a_list, b_list)
    r = np.zeros(n1 + n2 + 1, dtype=np.uint64)
    name, fn, mask = _dot_entry("auto", neg)
    rc = fn(_p(r), len(a_list), *mask, pa, pb, n1, n2)
    if rc:
        raise MpfftError(rc, f"{name}(K={len(a_list)}, n1={n1}, n2={n2})")
    return r


def dot_auto(a_list, b_list):
    """dot() with (depth, w) from dot_choose()"""
    return _dot_auto(None, a_list, b_list)


def sdot_auto(a_list, b_list, neg):
    """sdot() with (depth, w) from dot_choose()"""
    return _dot_auto(neg, a_list, b_list)


def _dot_stage(name, which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream):
    rc = getattr(lib(), "mpfft_" + name)(which, K, _ptr(d_a), _ptr(d_b), _ptr(d_r), n1, n2, depth, w, _ptr(ws), _nbytes(ws),
                                         _stream(stream))
    if rc:
        raise MpfftError(rc, f"mpfft_{name}({which})")


def dot_stage(which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream=None):
    """one stage for one term (d_a, d_b) on the K-term plan and workspace (tests)"""
    _dot_stage("dot_stage", which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream)


def sdot_stage(which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream=None):
    """one stage on the signed sum's workspace (tests): STAGE_SD_NEG, STAGE_SD_FIX, or a dot_stage stage"""
    _dot_stage("sdot_stage", which, K, d_a, d_b, d_r, n1, n2, depth, w, ws, stream)


def dot_stage_kernels(K, n1, n2, depth, w):
    """dict stage -> the kernels a K-term sum launches for it (the pointwise: the first term's kernel
    + the later terms')"""
    return _kernel_names(lib().mpfft_dot_stage_kernels, "mpfft_dot_stage_kernels", 640, STAGE_NAMES, K, n1, n2, depth, w)


def sdot_stage_kernels(K, neg, n1, n2, depth, w):
    """dot_stage_kernels' dict; with a negative term fwd_columns starts with the pre-pass kernel and
    combine ends with the correction's"""
    return _kernel_names(lib().mpfft_sdot_stage_kernels, "mpfft_sdot_stage_kernels", 768, STAGE_NAMES,
                         K, _neg_mask(neg), n1, n2, depth, w)


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
    return _kernel_names(lib().mpfft_precomp_stage_kernels, "mpfft_precomp_stage_kernels", 640, PRECOMP_STAGE_NAMES,
                         n1, n2, depth, w)


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


# ---- products modulo 2^B + 1 and 2^B - 1, B = 64 L (include/mpfft.h): three entry families with the
# same wrappers, written once in _ModFamily and bound to their public names below ----
STAGE_LOWCONV = 9   # mulmodw_stage: the low-word convolution d from the operands
M1_MUL, M1_SQR, M1_PRE = 0, 1, 2   # mulmodm1's plan kinds: multiply, square, multiply against a cached operand


class _ModFamily:
    """The wrappers of mpfft_<name>_* and the squares' mpfft_sqr<name[3:]>_*.
    extra: operands and result are L + extra limbs; kind: what the plan entries' last argument is made
    from (a flag, or one of M1_*); layout_keys: the words of workspace_layout; d_view: workspace_views
    also returns the low-word convolution"""

    def __init__(self, name, extra, kind, layout_keys, d_view=False):
        self.name, self.sq, self.extra, self.kind, self.layout_keys, self.d_view = \
            name, "sqr" + name[3:], extra, kind, layout_keys, d_view
        self.limbs = "L + %d" % extra if extra else "L"

    def _fn(self, entry, sq=False):
        return getattr(lib(), "mpfft_%s_%s" % (self.sq if sq else self.name, entry))

    def check_params(self, L, depth, w):
        return self._fn("check_params")(L, depth, w)

    def mul(self, a, b, depth, w):
        """a b mod 2^(64 L) +- 1 as a new uint64 array (host pointers); mod 2^B + 1: L + 1-limb fully reduced
        operands and result, mod 2^B - 1: L limbs, any operand value, the result fully reduced"""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        if len(a) != len(b) or len(a) < self.extra + 1:
            raise ValueError("operands are %s limbs each" % self.limbs)
        L = len(a) - self.extra
        r = np.zeros(len(a), dtype=np.uint64)
        rc = self._fn("ex")(_p(r), _p(a), _p(b), L, depth, w)
        if rc:
            raise MpfftError(rc, f"{self.name}(L={L}, depth={depth}, w={w})")
        return r

    def sqr(self, a, depth, w):
        """a^2 mod 2^(64 L) +- 1 (one forward transform)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        if len(a) < self.extra + 1:
            raise ValueError("the operand is %s limbs" % self.limbs)
        L = len(a) - self.extra
        r = np.zeros(len(a), dtype=np.uint64)
        rc = self._fn("ex", True)(_p(r), _p(a), L, depth, w)
        if rc:
            raise MpfftError(rc, f"{self.sq}(L={L}, depth={depth}, w={w})")
        return r

    def workspace_bytes(self, L, depth, w, kind=0):
        return int(self._fn("workspace_bytes")(L, depth, w, self.kind(kind)))

    def alloc_workspace(self, L, depth, w, kind=0, device="cuda"):
        import torch
        nb = self.workspace_bytes(L, depth, w, kind)
        if nb == 0:   # (or 1: a kind the family does not have, on valid parameters)
            raise MpfftError(self.check_params(L, depth, w) or 1, self.name + " workspace")
        return torch.empty(nb, dtype=torch.uint8, device=device)

    def device(self, d_r, d_a, d_b, L, depth, w, ws, stream=None):
        """d_r = d_a d_b mod 2^(64 L) +- 1 on the GPU; queued on `stream`, not synchronised.
        d_r may not be (mod 2^B - 1: overlap) an operand (it may be the next call's)."""
        rc = self._fn("device")(_ptr(d_r), _ptr(d_a), _ptr(d_b), L, depth, w, _ptr(ws), _nbytes(ws), _stream(stream))
        if rc:
            raise MpfftError(rc, "mpfft_%s_device" % self.name)

    def sqr_device(self, d_r, d_a, L, depth, w, ws, stream=None):
        rc = self._fn("device", True)(_ptr(d_r), _ptr(d_a), L, depth, w, _ptr(ws), _nbytes(ws), _stream(stream))
        if rc:
            raise MpfftError(rc, "mpfft_%s_device" % self.sq)

    def plan_info(self, L, depth, w):
        return _plan_info(self._fn("plan_info"), f"{self.name} plan(L={L}, depth={depth}, w={w})", L, depth, w)

    def workspace_layout(self, L, depth, w, kind=0):
        return _layout(self._fn("workspace_layout"), self.name + "_workspace_layout", self.layout_keys,
                       L, depth, w, self.kind(kind))

    def workspace_views(self, ws, L, depth, w, kind=0):
        """(digA, topA, cbA) views into a workspace tensor (slot-major): limbs (slots, l) int64, carry
        limbs int32, carry masks (slots, cbw) int64; mulmodw: and the low-word convolution d, (slots,)
        int32 (the words mod 2^32)."""
        import torch
        P = self.plan_info(L, depth, w)
        lay = self.workspace_layout(L, depth, w, kind)
        slots, l, cbw = lay["slots"], P["l"], lay["cbw"]
        u8 = ws.view(torch.uint8)
        dig = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
        top = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
        cb = u8[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
        if not self.d_view:
            return dig, top, cb
        return dig, top, cb, u8[lay["d"]:lay["d"] + slots * 4].view(torch.int32)

    def stage(self, which, d_a, d_b, d_r, L, depth, w, ws, kind=0, stream=None):
        rc = self._fn("stage")(which, _ptr(d_a), _ptr(d_b), _ptr(d_r), L, depth, w, self.kind(kind), _ptr(ws),
                               _nbytes(ws), _stream(stream))
        if rc:
            raise MpfftError(rc, f"mpfft_{self.name}_stage({which})")

    def stage_kernels(self, L, depth, w, kind=0):
        """dict stage -> the kernel a product mod 2^(64 L) +- 1 launches for it"""
        return _kernel_names(self._fn("stage_kernels"), "mpfft_%s_stage_kernels" % self.name, 512, STAGE_NAMES,
                             L, depth, w, self.kind(kind))

    def choose(self, L):
        """(depth, w) of least predicted time that are valid for this L."""
        d, w = ctypes.c_ulong(), ctypes.c_ulong()
        rc = self._fn("choose")(L, ctypes.byref(d), ctypes.byref(w))
        if rc:
            raise MpfftError(rc, f"{self.name}_choose(L={L})")
        return int(d.value), int(w.value)

    def next_size(self, min_L):
        """(L, depth, w): an efficient modulus size L >= min_L and its parameters."""
        L, d, w = ctypes.c_long(), ctypes.c_ulong(), ctypes.c_ulong()
        rc = self._fn("next_size")(min_L, ctypes.byref(L), ctypes.byref(d), ctypes.byref(w))
        if rc:
            raise MpfftError(rc, f"{self.name}_next_size({min_L})")
        return int(L.value), int(d.value), int(w.value)


def _flag(sqr):
    return int(bool(sqr))


# mod 2^B + 1 (mpfft_mulmod_*): operands and result are L + 1 limbs, fully reduced (0 <= a <= 2^B); the last
# argument of the plan entries is sqr
_MULMOD = _ModFamily("mulmod", 1, _flag, _LAYOUT_KEYS)
mulmod_check_params = _MULMOD.check_params
mulmod = _MULMOD.mul
sqrmod = _MULMOD.sqr
mulmod_workspace_bytes = _MULMOD.workspace_bytes
alloc_workspace_mulmod = _MULMOD.alloc_workspace
mulmod_device = _MULMOD.device
sqrmod_device = _MULMOD.sqr_device
mulmod_plan_info = _MULMOD.plan_info
mulmod_workspace_layout = _MULMOD.workspace_layout
mulmod_workspace_views = _MULMOD.workspace_views
mulmod_stage = _MULMOD.stage
mulmod_stage_kernels = _MULMOD.stage_kernels
mulmod_choose = _MULMOD.choose
mulmod_next_size = _MULMOD.next_size

# the same with the low-word CRT (mpfft_mulmodw_*): valid up to 2 bits1 + depth + 2 <= N + 32 (and from
# bits1 = 32 on); one layout word and one view more, d
_MULMODW = _ModFamily("mulmodw", 1, _flag, _LAYOUT_KEYS + ("d",), d_view=True)
mulmodw_check_params = _MULMODW.check_params
mulmodw = _MULMODW.mul
sqrmodw = _MULMODW.sqr
mulmodw_workspace_bytes = _MULMODW.workspace_bytes
alloc_workspace_mulmodw = _MULMODW.alloc_workspace
mulmodw_device = _MULMODW.device
sqrmodw_device = _MULMODW.sqr_device
mulmodw_plan_info = _MULMODW.plan_info
mulmodw_workspace_layout = _MULMODW.workspace_layout
mulmodw_workspace_views = _MULMODW.workspace_views
mulmodw_stage = _MULMODW.stage
mulmodw_stage_kernels = _MULMODW.stage_kernels
mulmodw_choose = _MULMODW.choose
mulmodw_next_size = _MULMODW.next_size

# mod 2^B - 1 (mpfft_mulmodm1_*): operands and result are L limbs; any operand value is valid, the result is
# fully reduced (never all-ones); the last argument of the plan entries is a kind M1_*
_MULMODM1 = _ModFamily("mulmodm1", 0, int, _LAYOUT_KEYS)
mulmodm1_check_params = _MULMODM1.check_params
mulmodm1 = _MULMODM1.mul
sqrmodm1 = _MULMODM1.sqr
mulmodm1_workspace_bytes = _MULMODM1.workspace_bytes
alloc_workspace_mulmodm1 = _MULMODM1.alloc_workspace
mulmodm1_device = _MULMODM1.device
sqrmodm1_device = _MULMODM1.sqr_device
mulmodm1_plan_info = _MULMODM1.plan_info
mulmodm1_workspace_layout = _MULMODM1.workspace_layout
mulmodm1_workspace_views = _MULMODM1.workspace_views
mulmodm1_stage = _MULMODM1.stage
mulmodm1_stage_kernels = _MULMODM1.stage_kernels
mulmodm1_choose = _MULMODM1.choose
mulmodm1_next_size = _MULMODM1.next_size


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
