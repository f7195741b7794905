#!/usr/bin/env python3
"""Record what a libmpfft.so decides, without a device: for every case below the plan, the
workspace size and layout, the stage kernels and the inverse-column schedule of the multiply,
the squaring counterparts for (n1, depth, w), the sqrt2 (mul6) plan of the two mul6 cases, and
the return codes of three invalid parameter sets.

    python3 scripts/dump_plans.py path/to/libmpfft.so > tests/golden/plans.json

tests/test_plan_golden.py compares the built library with the committed recording field by
field.  The recording is made from a build of the commit *before* a refactor of the planning
code, in a separate checkout -- never from the branch under test.

A second recording covers what the C ABI layer and the Python bindings decide for the other entry
families (mulmodw, mulmodm1, the cached operand, dot, sdot), the choosers' picks, the status codes
of the stage and device entries for null pointers, and the package's public names:

    python3 scripts/dump_plans.py --families path/to/libmpfft.so > tests/golden/family_answers.json

tests/test_family_golden.py compares it the same way; the same rule holds for where it is made
(the library's directory is the checkout's package directory: its __init__.py is loaded too).
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


# ---- the second recording: what the C ABI layer and the bindings decide for the other families ----
# (depth, w, L): tests/test_mulmodw_cpu.py's SHAPES and the three extra shapes of its kernel-name test
MULMODW_SHAPES = [(4, 8, 32), (5, 4, 75), (4, 8, 38), (5, 4, 76), (2, 16, 5), (6, 1, 88), (6, 64, 4120),
                  (5, 2048, 32780), (5, 4096, 65548), (14, 4, 1 << 24), (6, 3, 216), (9, 256, 1048576)]
MULMODW_CHOOSE = sorted({4, 5, 38, 1000, 33550336} | {1 << k for k in range(10, 25)})
MULMODW_NEXT = [1, 3, 1000, 10 ** 6, 1 << 24]
# tests/test_mulmodm1_cpu.py's SHAPES + FULL[6:] and the two extra shapes of its kernel-name test
MULMODM1_SHAPES = [(4, 4, 14), (4, 8, 30), (5, 64, 1021), (6, 64, 4088), (6, 1, 56), (6, 3, 184), (4, 4, 7), (6, 64, 2048),
                   (2, 16, 1), (2, 32, 1), (6, 192, 12280), (6, 512, 32760), (5, 1024, 16381), (5, 2048, 32765),
                   (5, 4096, 65533), (14, 8, 33550336), (9, 256, 1048496), (8, 1024, 1048536)]
MULMODM1_NEXT = [1, 1000, 5000, 10 ** 6, 33550336]
# (K, depth, w, n): K in (1, 2, 64) on test_dot_cpu.py's test_workspace_holds_three_disjoint_arrays shapes,
# thinned to K = 2 everywhere and K = 1, 64 on the largest and the smallest plan
_DOT_SHAPES = [(15, 4, 20000000), (7, 1024, 131000), (8, 512, 140000), (11, 8, 5000), (9, 2, 120)]
DOT_CASES = [(2,) + s for s in _DOT_SHAPES] + [(K,) + s for K in (1, 64) for s in (_DOT_SHAPES[0], _DOT_SHAPES[4])]
DOT_CHOOSE = [(1, 1, 1), (2, 7, 3), (3, 1000, 1000), (4, 100000, 60000), (64, 3000000, 3000000), (2, 20000000, 20000000)]
# (K, neg) of tests/test_sdot_cpu.py: a mask bit at or above K, a mask inside K
SDOT_MASKS = [(1, 2), (1, 3), (2, 4), (2, 7), (3, 1 << 3), (4, 1 << 63), (63, 1 << 63), (5, (1 << 64) - 1),
              (1, 1), (2, 3), (3, 5), (64, (1 << 64) - 1), (64, 1 << 63), (7, 0)]
CHOOSE_SIZES = [1, 2, 16, 100, 1000, 16384, 10 ** 5, 261952, 10 ** 6, 15625000, 20312500, 156250000]
STAGE_DRIVEN, STAGE_ACC = 0x100, 0x200

_I, _VP, _U64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64
_LP, _ULP, _SZP = ctypes.POINTER(_L), ctypes.POINTER(_UL), ctypes.POINTER(_SZ)


def _load_families(path):
    lib = ctypes.CDLL(path)
    mod, text, dot = [_L, _UL, _UL], [ctypes.c_char_p, _SZ], [_L, _L, _L, _UL, _UL]
    mul, tail = [_L, _L, _UL, _UL], [_VP, _SZ, _VP]
    sig = [("choose", _I, [_L, _L, _ULP, _ULP]),
           ("precomp_bytes", _SZ, mul), ("mul_precomp_workspace_bytes", _SZ, mul), ("precomp_stage_kernels", _I, mul + text),
           ("mulmodm1_precomp_bytes", _SZ, mod),
           ("dot_check_params", _I, dot), ("dot_plan_info", _I, dot + [_LP]), ("dot_workspace_bytes", _SZ, dot),
           ("dot_workspace_layout", _I, dot + [_SZP]), ("dot_stage_kernels", _I, dot + text),
           ("dot_choose", _I, [_L, _L, _L, _ULP, _ULP]),
           ("sdot_check_params", _I, [_L, _U64] + dot[1:]), ("sdot_workspace_bytes", _SZ, dot),
           ("sdot_workspace_layout", _I, dot + [_SZP]), ("sdot_stage_kernels", _I, [_L, _U64] + dot[1:] + text),
           # stage and device entries: every pointer a void *
           ("stage", _I, [_I, _VP, _VP, _VP] + mul + tail), ("sqr_stage", _I, [_I, _VP, _VP] + mod + tail),
           ("precomp_stage", _I, [_I, _VP, _SZ, _VP] + mul + tail),
           ("mul_precomp_stage", _I, [_I, _VP, _VP, _SZ, _VP] + mul + tail),
           ("dot_stage", _I, [_I, _L, _VP, _VP, _VP] + mul + tail), ("sdot_stage", _I, [_I, _L, _VP, _VP, _VP] + mul + tail),
           ("mul_device", _I, [_VP, _VP, _L, _VP, _L, _UL, _UL] + tail),
           ("mul6_device", _I, [_VP, _VP, _L, _VP, _L, _UL, _UL] + tail),
           ("sqr_device", _I, [_VP, _VP] + mod + tail),
           ("precomp_device", _I, [_VP, _SZ, _VP] + mul + tail),
           ("mul_precomp_device", _I, [_VP, _VP, _L, _VP, _SZ, _L, _UL, _UL] + tail),
           ("mulmodm1_precomp_device", _I, [_VP, _SZ, _VP] + mod + tail),
           ("mulmodm1_mul_precomp_device", _I, [_VP, _VP, _VP, _SZ] + mod + tail),
           ("dot_device", _I, [_VP, _L, _VP, _VP] + mul + tail), ("sdot_device", _I, [_VP, _L, _U64, _VP, _VP] + mul + tail)]
    for fam, sq in (("mulmod", "sqrmod"), ("mulmodw", "sqrmodw"), ("mulmodm1", "sqrmodm1")):
        sig += [(fam + "_check_params", _I, mod), (fam + "_plan_info", _I, mod + [_LP]),
                (fam + "_workspace_bytes", _SZ, mod + [_I]), (fam + "_workspace_layout", _I, mod + [_I, _SZP]),
                (fam + "_stage_kernels", _I, mod + [_I] + text), (fam + "_choose", _I, [_L, _ULP, _ULP]),
                (fam + "_next_size", _I, [_L, _LP, _ULP, _ULP]),
                (fam + "_stage", _I, [_I, _VP, _VP, _VP] + mod + [_I] + tail),
                (fam + "_device", _I, [_VP, _VP, _VP] + mod + tail), (sq + "_device", _I, [_VP, _VP] + mod + tail)]
    for name, res, args in sig:
        f = getattr(lib, "mpfft_" + name)
        f.restype, f.argtypes = res, args
    return lib


def _picked(fn, ctypes_out, *args):
    """a chooser's answer: (L,) depth, w"""
    out = [t() for t in ctypes_out]
    rc = fn(*args, *[ctypes.byref(o) for o in out])
    return {"rc": rc, "out": [int(o.value) for o in out] if rc == 0 else None}


def _mod_family(lib, fam, shapes, nlay, variants, choose, next_sizes, rejects):
    """{case: {entry: result}} of one mod family; `variants`: the values of its last argument (sqr / kind)"""
    f = lambda entry: getattr(lib, "mpfft_%s_%s" % (fam, entry))
    out = {}
    for depth, w, L in shapes:
        a = (L, depth, w)
        e = {"check_params": f("check_params")(*a), "plan_info": _ints(f("plan_info"), _L, 10, *a)}
        for v in variants:
            e["workspace_bytes %d" % v] = f("workspace_bytes")(*a, v)
            e["workspace_layout %d" % v] = _ints(f("workspace_layout"), _SZ, nlay, *a, v)
            e["stage_kernels %d" % v] = _text(f("stage_kernels"), *a, v)
        if fam == "mulmodm1":
            e["precomp_bytes"] = lib.mpfft_mulmodm1_precomp_bytes(*a)
        out["%s depth=%d w=%d L=%d" % (fam, depth, w, L)] = e
    out[fam + " choose"] = {"L=%d" % L: _picked(f("choose"), (_UL, _UL), L) for L in choose}
    out[fam + " next_size"] = {"m=%d" % m: _picked(f("next_size"), (_L, _UL, _UL), m) for m in next_sizes}
    rej = {}
    for L, depth, w in rejects:
        rej["check_params L=%d depth=%d w=%d" % (L, depth, w)] = f("check_params")(L, depth, w)
        for v in variants:
            rej["workspace_bytes L=%d depth=%d w=%d %d" % (L, depth, w, v)] = f("workspace_bytes")(L, depth, w, v)
    out[fam + " rejects"] = rej
    return out


def _one_step_past(full):
    """(L + g, depth, w) of the shapes at their largest bits1: one granularity step too large"""
    return [(L + max(1, (2 << depth) // 64), depth, w) for depth, w, L in full]


def _stage_codes(fn, head, tail):
    """fn(stage, *head, *tail) for stage 0..12 plain, | STAGE_DRIVEN and | STAGE_ACC: null pointers and
    ws_bytes = 0, so every call returns from an argument check"""
    return {name: [fn(st | flag, *head, *tail) for st in range(13)]
            for name, flag in (("plain", 0), ("driven", STAGE_DRIVEN), ("acc", STAGE_ACC))}


def _argument_checks(lib):
    """The codes of the stage and device entries for null pointers and no workspace.  Not recorded:
    the mpfft_shard_* stages (they take a descriptor, and mpfft_shard_stage clears the HIP error
    state before it looks at the stage) and mpfft_mul_multi_device (multi.hip)."""
    ws0, mul, mod, bad = (None, 0, None), (300, 300, 10, 3), (4088, 6, 64), (0, 9, 2)
    p = _VP(256)   # a pointer that is not null and is never followed: the workspace check comes first
    out = {"mpfft_stage": _stage_codes(lib.mpfft_stage, (None, None, None) + mul, ws0),
           "mpfft_sqr_stage": _stage_codes(lib.mpfft_sqr_stage, (None, None, 300, 10, 3), ws0),
           "mpfft_precomp_stage": _stage_codes(lib.mpfft_precomp_stage, (None, 0, None) + mul, ws0),
           "mpfft_mul_precomp_stage": _stage_codes(lib.mpfft_mul_precomp_stage, (None, None, 0, None) + mul, ws0),
           "mpfft_dot_stage": _stage_codes(lib.mpfft_dot_stage, (2, None, None, None) + mul, ws0),
           "mpfft_sdot_stage": _stage_codes(lib.mpfft_sdot_stage, (2, None, None, None) + mul, ws0)}
    for fam, variants in (("mulmod", (0, 1)), ("mulmodw", (0, 1)), ("mulmodm1", (0, 1, 2, 3))):
        fn = getattr(lib, "mpfft_%s_stage" % fam)
        for v in variants:
            out["mpfft_%s_stage %d" % (fam, v)] = _stage_codes(fn, (None, None, None) + mod + (v,), ws0)
    dev = {}
    for name, shape in (("valid", mul), ("invalid", (0, 300, 10, 3))):
        n1, n2, depth, w = shape
        dev["mpfft_mul_device " + name] = lib.mpfft_mul_device(None, None, n1, None, n2, depth, w, *ws0)
        dev["mpfft_mul6_device " + name] = lib.mpfft_mul6_device(None, None, n1, None, n2, depth, w, *ws0)
        dev["mpfft_sqr_device " + name] = lib.mpfft_sqr_device(None, None, n1, depth, w, *ws0)
        dev["mpfft_precomp_device " + name] = lib.mpfft_precomp_device(None, 0, None, *shape, *ws0)
        dev["mpfft_mul_precomp_device " + name] = lib.mpfft_mul_precomp_device(None, None, n1, None, 0, n2, depth, w, *ws0)
        for K, neg in ((2, 1), (2, 4), (0, 0)):   # the mask inside K, past K, no such K
            dev["mpfft_dot_device K=%d null terms %s" % (K, name)] = lib.mpfft_dot_device(None, K, None, None, *shape, *ws0)
            dev["mpfft_dot_device K=%d %s" % (K, name)] = lib.mpfft_dot_device(p, K, p, p, *shape, *ws0)
            dev["mpfft_sdot_device K=%d neg=%d null terms %s" % (K, neg, name)] = \
                lib.mpfft_sdot_device(None, K, neg, None, None, *shape, *ws0)
            dev["mpfft_sdot_device K=%d neg=%d %s" % (K, neg, name)] = lib.mpfft_sdot_device(p, K, neg, p, p, *shape, *ws0)
    for name, shape in (("valid", mod), ("invalid", (4087, 6, 64))):
        for fam, sq in (("mulmod", "sqrmod"), ("mulmodw", "sqrmodw"), ("mulmodm1", "sqrmodm1")):
            dev["mpfft_%s_device %s" % (fam, name)] = getattr(lib, "mpfft_%s_device" % fam)(None, None, None, *shape, *ws0)
            dev["mpfft_%s_device %s" % (sq, name)] = getattr(lib, "mpfft_%s_device" % sq)(None, None, *shape, *ws0)
        dev["mpfft_mulmodm1_precomp_device " + name] = lib.mpfft_mulmodm1_precomp_device(None, 0, None, *shape, *ws0)
        dev["mpfft_mulmodm1_mul_precomp_device " + name] = lib.mpfft_mulmodm1_mul_precomp_device(None, None, None, 0, *shape, *ws0)
    out["device entries"] = dev
    return out


def public_names(package_init):
    """the sorted public names a fresh load of the package's __init__.py binds, imported modules excluded"""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("_mpfft_surface", package_init)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return sorted(k for k, v in vars(mod).items() if not k.startswith("_") and not isinstance(v, types.ModuleType))


def dump_families(path):
    """{case name: {entry: result}} of the entry families the first recording leaves out: mulmodw, mulmodm1,
    the cached operand, dot and sdot, mpfft_choose, the argument checks of the stage and device entries,
    and the public names of the package next to the library"""
    import os
    lib = _load_families(path)
    w_full, m1_full = MULMODW_SHAPES[2:9], MULMODM1_SHAPES[:6] + MULMODM1_SHAPES[10:16]
    out = _mod_family(lib, "mulmodw", MULMODW_SHAPES, 9, (0, 1), MULMODW_CHOOSE + [3, 1 << 40], MULMODW_NEXT + [0],
                      [(4119, 6, 64), (0, 6, 64), (32, 1, 32), (14, 4, 3), (14, 4, 4), (62, 6, 64), (64, 6, 64),
                       (1000, 7, 4096), (39, 4, 8)] + _one_step_past(w_full))
    out.update(_mod_family(lib, "mulmodm1", MULMODM1_SHAPES, 8, (0, 1, 2), [L for _, _, L in MULMODM1_SHAPES] + [1 << 40],
                           MULMODM1_NEXT + [0],
                           [(4087, 6, 64), (0, 6, 64), (14, 1, 32), (14, 31, 1), (14, 4, 3), (1000, 7, 4096), (15, 4, 4)]
                           + _one_step_past(m1_full)))
    out["mulmodm1 rejects"]["workspace_bytes L=14 depth=4 w=4 3"] = lib.mpfft_mulmodm1_workspace_bytes(14, 4, 4, 3)
    for L, depth, w in _one_step_past(m1_full):
        out["mulmodm1 rejects"]["precomp_bytes L=%d depth=%d w=%d" % (L, depth, w)] = lib.mpfft_mulmodm1_precomp_bytes(L, depth, w)
    for depth, w, n1, n2 in CASES:
        a = (n1, n2, depth, w)
        out["precomp depth=%d w=%d n1=%d n2=%d" % (depth, w, n1, n2)] = {
            "precomp_bytes": lib.mpfft_precomp_bytes(*a),
            "mul_precomp_workspace_bytes": lib.mpfft_mul_precomp_workspace_bytes(*a),
            "precomp_stage_kernels": _text(lib.mpfft_precomp_stage_kernels, *a)}
    for K, depth, w, n in DOT_CASES:
        a = (K, n, n, depth, w)
        out["dot K=%d depth=%d w=%d n=%d" % (K, depth, w, n)] = {
            "check_params": lib.mpfft_dot_check_params(*a), "plan_info": _ints(lib.mpfft_dot_plan_info, _L, 10, *a),
            "workspace_bytes": lib.mpfft_dot_workspace_bytes(*a),
            "workspace_layout": _ints(lib.mpfft_dot_workspace_layout, _SZ, 11, *a),
            "stage_kernels": _text(lib.mpfft_dot_stage_kernels, *a)}
        out["sdot K=%d depth=%d w=%d n=%d" % (K, depth, w, n)] = {
            "check_params": lib.mpfft_sdot_check_params(K, 1, n, n, depth, w),
            "workspace_bytes": lib.mpfft_sdot_workspace_bytes(*a),
            "workspace_layout": _ints(lib.mpfft_sdot_workspace_layout, _SZ, 13, *a),
            "stage_kernels neg=0": _text(lib.mpfft_sdot_stage_kernels, K, 0, n, n, depth, w),
            "stage_kernels neg=1": _text(lib.mpfft_sdot_stage_kernels, K, 1, n, n, depth, w)}
    out["dot choose"] = {"K=%d n1=%d n2=%d" % c: _picked(lib.mpfft_dot_choose, (_UL, _UL), *c)
                         for c in DOT_CHOOSE + [(0, 100, 100), (65, 100, 100), (2, 10 ** 12, 10 ** 12)]}
    out["sdot masks"] = {"K=%d neg=%d" % (K, neg): lib.mpfft_sdot_check_params(K, neg, 100, 100, 9, 2) for K, neg in SDOT_MASKS}
    out["choose"] = {"n1=%d n2=%d" % (n1, n2): _picked(lib.mpfft_choose, (_UL, _UL), n1, n2)
                     for n in CHOOSE_SIZES for n1, n2 in sorted({(n, n), (n, max(1, n // 7)), (n, 3)})}
    out["choose"]["n1=%d n2=%d" % (10 ** 12, 10 ** 12)] = _picked(lib.mpfft_choose, (_UL, _UL), 10 ** 12, 10 ** 12)
    out["argument checks"] = _argument_checks(lib)
    out["public names"] = public_names(os.path.join(os.path.dirname(os.path.abspath(path)), "__init__.py"))
    return out


def write_families(rec, f):
    """one case per line: the kernel-name strings make up most of the file, the rest stays compact"""
    f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(rec[k], sort_keys=True, separators=(",", ":")))
                               for k in sorted(rec)) + "\n}\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--families":
        write_families(dump_families(sys.argv[2]), sys.stdout)
    elif len(sys.argv) == 2:
        json.dump(dump(sys.argv[1]), sys.stdout, indent=1, sort_keys=True)
        sys.stdout.write("\n")
    else:
        sys.exit(__doc__)
