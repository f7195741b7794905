"""Small matrix products (mpfft_matmul_*, include/mpfft.h): R = X Y, X m x k with entries of n1 limbs, Y
k x p with entries of n2 limbs, R m x p with entries of n1 + n2 + 1 limbs, on the dot plan at K = k
(dot_choose(k, n1, n2), dot_plan_info, dot_max_limbs of the package): every operand forward-transformed
once into a cache in the workspace, one pointwise sum and one inverse per result entry.  Matrices are
row-major lists (or lists of rows) of tensors / limb arrays.

The Python mirror of that entry family, a submodule of the package as sharded.py is:
    from mpir_fft_amd.matmul import matmul_device, alloc_workspace_matmul
The ctypes signatures of the entries are in the package's _signatures table with all the others.
"""
import ctypes

import numpy as np

from . import (MpfftError, STAGE_NAMES, _DOT_LAYOUT_KEYS, _kernel_names, _layout, _nbytes, _ptr, _ptr_array, _stream,
               lib)

MM_MAX = 4
STAGE_MM_STORE = 12       # matmul_stage: the row arrays of operand 0 (a cache of X) or 1 -> cache ea[0]
STAGE_MM_POINTWISE = 13   # matmul_stage: C <- sum_i cache ea[i] * cache eb[i] (| STAGE_ACC: C <- C + the sum)


def matmul_check_params(m, k, p, n1, n2, depth, w):
    return lib().mpfft_matmul_check_params(m, k, p, n1, n2, depth, w)


def matmul_workspace_bytes(m, k, p, n1, n2, depth, w):
    return int(lib().mpfft_matmul_workspace_bytes(m, k, p, n1, n2, depth, w))


def alloc_workspace_matmul(m, k, p, n1, n2, depth, w, device="cuda"):
    import torch
    nb = matmul_workspace_bytes(m, k, p, n1, n2, depth, w)
    if nb == 0:
        raise MpfftError(matmul_check_params(m, k, p, n1, n2, depth, w), "matmul workspace")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def matmul_workspace_layout(m, k, p, n1, n2, depth, w):
    """dot_workspace_layout(k, ...)'s entries, then "cache0" (byte offset of cache 0), "stride" (bytes between
    caches) and "ncache" (m k + k p; X[i][t] is cache i k + t, Y[t][j] cache m k + t p + j)"""
    return _layout(lib().mpfft_matmul_workspace_layout, "matmul_workspace_layout",
                   _DOT_LAYOUT_KEYS + ("cache0", "stride", "ncache"), m, k, p, n1, n2, depth, w)


def _flat(mat, rows, cols, what):
    """a rows x cols matrix given as a flat row-major sequence or as a sequence of rows -> a flat list"""
    mat = list(mat)
    if len(mat) == rows and rows * cols != rows:
        mat = [e for row in mat for e in row]
    elif len(mat) == rows and cols == 1 and isinstance(mat[0], (list, tuple)):
        mat = [e for row in mat for e in row]
    if len(mat) != rows * cols:
        raise ValueError(f"{what}: {rows} x {cols} entries")
    return mat


def matmul_device(d_rs, m, k, p, d_xs, d_ys, n1, n2, depth, w, ws, stream=None):
    """d_rs[i p + j][:n1 + n2 + 1] = sum_t d_xs[i k + t][:n1] * d_ys[t p + j][:n2], all tensors on the GPU
    (row-major lists, or lists of rows; an operand tensor may appear more than once); queued on `stream`,
    not synchronised."""
    d_rs, d_xs, d_ys = _flat(d_rs, m, p, "results"), _flat(d_xs, m, k, "X"), _flat(d_ys, k, p, "Y")
    rc = lib().mpfft_matmul_device(_ptr_array(d_rs), m, k, p, _ptr_array(d_xs), _ptr_array(d_ys), n1, n2, depth, w,
                                   _ptr(ws), _nbytes(ws), _stream(stream))
    if rc:
        raise MpfftError(rc, "mpfft_matmul_device")


def _host_matrices(xs, ys, m, k, p):
    xs = [np.ascontiguousarray(a, dtype=np.uint64) for a in _flat(xs, m, k, "X")]
    ys = [np.ascontiguousarray(b, dtype=np.uint64) for b in _flat(ys, k, p, "Y")]
    n1, n2 = len(xs[0]), len(ys[0])
    if any(len(a) != n1 for a in xs) or any(len(b) != n2 for b in ys):
        raise ValueError("every entry of X of n1 limbs, every entry of Y of n2 limbs")
    rs = [np.zeros(n1 + n2 + 1, dtype=np.uint64) for _ in range(m * p)]
    arr = lambda v: (ctypes.c_void_p * len(v))(*[a.ctypes.data for a in v])
    return xs, ys, rs, arr(xs), arr(ys), arr(rs), n1, n2


def matmul(xs, ys, m, k, p, depth, w):
    """X Y as a row-major list of m p new uint64 arrays of n1 + n2 + 1 limbs (host pointers, mpfft_matmul_ex)"""
    xs, ys, rs, px, py, pr, n1, n2 = _host_matrices(xs, ys, m, k, p)
    rc = lib().mpfft_matmul_ex(pr, m, k, p, px, py, n1, n2, depth, w)
    if rc:
        raise MpfftError(rc, f"matmul(m={m}, k={k}, p={p}, n1={n1}, n2={n2}, depth={depth}, w={w})")
    return rs


def matmul_auto(xs, ys, m, k, p):
    """matmul() with (depth, w) from dot_choose(k, n1, n2)"""
    xs, ys, rs, px, py, pr, n1, n2 = _host_matrices(xs, ys, m, k, p)
    rc = lib().mpfft_matmul_auto(pr, m, k, p, px, py, n1, n2)
    if rc:
        raise MpfftError(rc, f"matmul_auto(m={m}, k={k}, p={p}, n1={n1}, n2={n2})")
    return rs


def matmul_stage_kernels(m, k, p, n1, n2, depth, w):
    """dict stage -> the kernels a matrix product launches for it (the pointwise: what writes the caches +
    what forms a result entry's sum)"""
    return _kernel_names(lib().mpfft_matmul_stage_kernels, "mpfft_matmul_stage_kernels", 768, STAGE_NAMES,
                         m, k, p, n1, n2, depth, w)


def matmul_stage(which, m, k, p, d_a, d_b, d_r, n1, n2, depth, w, ws, ea=(), eb=(), stream=None):
    """one stage on the matrix product's workspace (tests): STAGE_MM_STORE (cache ea[0]), STAGE_MM_POINTWISE
    (the sum over the cache pairs ea[i], eb[i]; | STAGE_ACC), or a dot_stage stage at K = k"""
    ea, eb = list(ea), list(eb)
    pa = (ctypes.c_int * max(len(ea), 1))(*ea)
    pb = (ctypes.c_int * max(len(eb), 1))(*eb)
    rc = lib().mpfft_matmul_stage(which, m, k, p, _ptr(d_a), _ptr(d_b), _ptr(d_r), n1, n2, depth, w, _ptr(ws), _nbytes(ws),
                                  _stream(stream), len(ea), pa, pb)
    if rc:
        raise MpfftError(rc, f"mpfft_matmul_stage({which})")
