"""The bindings' signature table (mpir-fft_amd/__init__.py _signatures) against include/mpfft.h: beside
test_library_cpu.py's test_exports_every_declared_symbol, and parsing the header as it does.  ctypes
converts arguments by that table alone, so a missing entry or a wrong length corrupts a call silently.
No device is touched.
"""
import os
import re

from test_library_cpu import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# declared functions the bindings leave out on purpose: {name: reason}
UNBOUND = {}


def declared_prototypes():
    """{function: number of parameters} of every prototype in include/mpfft.h"""
    src = open(os.path.join(ROOT, "include", "mpfft.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"^\s*(?:void|int|long|size_t|const char \*)\s*\*?\s*(\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M)
    return {name: 0 if args.strip() in ("", "void") else args.count(",") + 1 for name, args in protos}


def test_signature_table_matches_the_header(mp):
    """every declared function has one entry in the table, with as many argtypes as the prototype has
    parameters, and lib() applied the table as it stands"""
    protos = declared_prototypes()
    assert sorted(protos) == declared_functions()
    assert protos["mpfft_version"] == 0 and protos["new_mpn_mul"] == 7 and protos["mpfft_sdot_device"] == 12
    table = mp._signatures()
    names = [name for name, _, _ in table]
    assert len(set(names)) == len(names)
    assert not set(names) - set(protos), sorted(set(names) - set(protos))
    for name in protos:
        if name not in UNBOUND:
            assert name in names, name
    for name, _, argtypes in table:
        assert len(argtypes) == protos[name], (name, len(argtypes), protos[name])
    lib = mp.lib()
    for name, restype, argtypes in table:
        f = getattr(lib, name)
        assert f.restype == restype and list(f.argtypes) == list(argtypes), name
