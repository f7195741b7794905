#!/bin/bash
# Build mutants of libmpfft that each flip one sign inside a carry, top or wrap branch of a
# transform pass, to show that tests/test_gpu_stage_adversarial.py bites where the random-operand
# stage test (tests/test_gpu_parity.py::test_stages_exact) may not.  A mutant computes wrong values
# only: no address, bound, launch parameter or barrier is touched.
#
#   wave_canon  wave.hpp wv_canon, the |top| <= 2 ripple: the last fix-up after the wrap (+1 / -1)
#               has its signs swapped                                   (k_lpass / k_wpass, k_wscale)
#   wave_top    wave.hpp wv_load_digits: the carry limb enters limb 0 with the wrong sign
#   rp_carry    rkernels.hpp rp_decode: the carry out of adding a limb's incoming carry enters the
#               pair overflow with the wrong sign                       (k_rpass, k_rpair, k_rchain)
#
# Output: mpir-fft_amd/libmpfft_mut_<name>.so (built from copies under $TMPDIR; csrc/ untouched).
# Then, on the GPU: python scripts/mutant_stage_check.py  (log: profiles/r10/mutants.txt)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
for NAME in ${@:-wave_canon wave_top rp_carry}; do
    T=$(mktemp -d "${TMPDIR:-/tmp}/mpfft_mut_$NAME.XXXXXX")
    mkdir -p $T/mpir-fft_amd $T/include
    cp -r $ROOT/mpir-fft_amd/csrc $T/mpir-fft_amd/ && cp $ROOT/include/mpfft.h $T/include/
    rm -rf $T/mpir-fft_amd/csrc/build*
    python3 - $T/mpir-fft_amd/csrc $NAME <<'PY'
import sys
d, name = sys.argv[1], sys.argv[2]
MUT = {
    "wave_canon": ("wave.hpp", "        else if (m == 0) f[u] = sub ? f[u] + 1 : f[u] - 1;",
                   "        else if (m == 0) f[u] = sub ? f[u] - 1 : f[u] + 1;   // MUTANT", 0),
    "wave_top": ("wave.hpp", "const i64 cl = (i64)((pp >> b) & 1) - (i64)((pn >> b) & 1) + r.top;",
                 "const i64 cl = (i64)((pp >> b) & 1) - (i64)((pn >> b) & 1) - r.top;   // MUTANT", 0),
    # the second occurrence: rp_decode (the first is the rotated load rp_decode_rot)
    "rp_carry": ("rkernels.hpp", "            x[i][r].h = c1 + cc;", "            x[i][r].h = c1 - cc;   // MUTANT", 1),
}
f, a, b, nth = MUT[name]
s = open(d + "/" + f).read()
assert s.count(a) == nth + 1, (name, s.count(a))
i = -1
for _ in range(nth + 1):
    i = s.index(a, i + 1)
open(d + "/" + f, "w").write(s[:i] + b + s[i + len(a):])
PY
    make -s -C $T/mpir-fft_amd/csrc -j8 >/dev/null
    cp $T/mpir-fft_amd/libmpfft.so $ROOT/mpir-fft_amd/libmpfft_mut_$NAME.so
    rm -rf $T
    echo "built $ROOT/mpir-fft_amd/libmpfft_mut_$NAME.so"
done
