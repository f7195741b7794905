#!/usr/bin/env python3
"""Record what a libmpfft.so decides, without a device: for every case below the plan, the
workspace size and layout, the stage kernels and the inverse-column schedule of the multiply,
the squaring counterparts for (n1, depth, w), the sqrt2 (mul6) plan of the two mul6 cases, and
the return codes of three invalid parameter sets.

    python3 scripts/dump_plans.py path/to/libmpfft.so > tests/golden/plans.json

tests/test_plan_golden.py compares the built library with the committed recording field by
field.  The recording is made from a build of the commit *before* a refactor of the planning
code, in a separate checkout -- never from the branch under test.
"""
import ctypes
import json
import sys

# (depth, w, n1, n2)
CASES = [
    # bench.py's C0-C4
    (11, 1, 16384, 16384), (11, 8, 261952, 261952), (15, 4, 15625000, 15625000),
    (15, 4, 20312500, 20312500), (17, 2, 156250000, 156250000),
    # tests/test_tail_fold.py's CASES, n1 = n2 = limbs
    (6, 1024, 16710, 16710), (7, 1024, 66842, 66842), (7, 2048, 133689, 133689),
    (7, 512, 33419, 33419), (9, 256, 262648, 262648), (9, 512, 525316, 525316),
    (9, 128, 131314, 131314), (11, 64, 1100000, 1100000), (11, 128, 2105444, 2105444),
    (9, 128, 147564, 147564), (9, 256, 328179, 328179), (9, 512, 656383, 656383),
    (7, 512, 49801, 49801), (9, 256, 197117, 197117), (9, 512, 394249, 394249),
    (7, 1024, 82570, 82570),
    # the smoke shape, small wave plans, an l = 512 plan (big without rpass), an unequal pair
    (9, 2, 120, 97), (11, 8, 5000, 5000), (9, 64, 3000, 2000), (9, 64, 30000, 30000),
    (15, 4, 20312500, 9000000),
]
CASES6 = [(8, 1, 700, 500), (14, 1, 3142656, 3142656)]
# (n, depth, w) of tests/test_sqr_cpu.py's parameter errors: EINVAL, ETOOBIG, EUNSUPPORTED
ERRORS = [(0, 9, 2), (100000, 6, 1), (100, 13, 64)]

_L, _UL, _SZ = ctypes.c_long, ctypes.c_ulong, ctypes.c_size_t
_BUF = 1 << 20


def _load(path):
    lib = ctypes.CDLL(path)
    mul, sqr = [_L, _L, _UL, _UL], [_L, _UL, _UL]
    text = [ctypes.c_char_p, _SZ]
    for name, res, args in (
            ("check_params", ctypes.c_int, mul), ("check_params6", ctypes.c_int, mul),
            ("plan_info", ctypes.c_int, mul + [ctypes.POINTER(_L)]),
            ("plan_info6", ctypes.c_int, mul + [ctypes.POINTER(_L)]),
            ("workspace_bytes", _SZ, mul), ("workspace_bytes6", _SZ, mul),
            ("workspace_layout", ctypes.c_int, mul + [ctypes.POINTER(_SZ)]),
            ("stage_kernels", ctypes.c_int, mul + text),
            ("inv_columns_schedule", ctypes.c_int, mul + text),
            ("sqr_workspace_bytes", _SZ, sqr),
            ("sqr_workspace_layout", ctypes.c_int, sqr + [ctypes.POINTER(_SZ)]),
            ("sqr_stage_kernels", ctypes.c_int, sqr + text)):
        f = getattr(lib, "mpfft_" + name)
        f.restype, f.argtypes = res, args
    return lib


def _ints(fn, ctype, count, *args):
    out = (ctype * count)()
    rc = fn(*args, out)
    return {"rc": rc, "out": list(out) if rc == 0 else None}


def _text(fn, *args):
    buf = ctypes.create_string_buffer(_BUF)
    rc = fn(*args, buf, _BUF)
    return {"rc": rc, "out": buf.value.decode() if rc == 0 else None}


def _mul(lib, n1, n2, depth, w):
    a = (n1, n2, depth, w)
    return {"check_params": lib.mpfft_check_params(*a),
            "plan_info": _ints(lib.mpfft_plan_info, _L, 10, *a),
            "workspace_bytes": lib.mpfft_workspace_bytes(*a),
            "workspace_layout": _ints(lib.mpfft_workspace_layout, _SZ, 8, *a),
            "stage_kernels": _text(lib.mpfft_stage_kernels, *a),
            "inv_columns_schedule": _text(lib.mpfft_inv_columns_schedule, *a)}


def _sqr(lib, n, depth, w):
    a = (n, depth, w)
    return {"sqr_workspace_bytes": lib.mpfft_sqr_workspace_bytes(*a),
            "sqr_workspace_layout": _ints(lib.mpfft_sqr_workspace_layout, _SZ, 8, *a),
            "sqr_stage_kernels": _text(lib.mpfft_sqr_stage_kernels, *a)}


def dump(path):
    """{case name: {entry: result}} of the library at `path`"""
    lib = _load(path)
    out = {}
    for depth, w, n1, n2 in CASES:
        out["mul depth=%d w=%d n1=%d n2=%d" % (depth, w, n1, n2)] = {**_mul(lib, n1, n2, depth, w),
                                                                     **_sqr(lib, n1, depth, w)}
    for depth, w, n1, n2 in CASES6:
        a = (n1, n2, depth, w)
        out["mul6 depth=%d w=%d n1=%d n2=%d" % (depth, w, n1, n2)] = {
            "check_params6": lib.mpfft_check_params6(*a),
            "plan_info6": _ints(lib.mpfft_plan_info6, _L, 10, *a),
            "workspace_bytes6": lib.mpfft_workspace_bytes6(*a)}
    for n, depth, w in ERRORS:
        out["error n=%d depth=%d w=%d" % (n, depth, w)] = {**_mul(lib, n, n, depth, w), **_sqr(lib, n, depth, w)}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    json.dump(dump(sys.argv[1]), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
