"""CPU test of bench.py's --dump-outputs writer: the product limbs leave as float64 files of
32-bit halves (exact), a fixed seeded sample and per-chunk sums over the whole product, the
same from call to call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(d):
    return np.load(os.path.join(d, "product_sample.npy")), np.load(os.path.join(d, "product_chunk_sums.npy"))


def test_dump_outputs_exact_and_repeatable(tmp_path):
    import bench
    n = 3 * bench.DUMP_CHUNK + 17          # not a multiple of the chunk, fewer limbs than the sample
    prod = np.random.default_rng(7).integers(0, 1 << 64, size=n, dtype=np.uint64)
    prod[0], prod[-1] = np.uint64((1 << 64) - 1), np.uint64(1 << 63)
    bench.dump_outputs(str(tmp_path / "a"), prod)
    bench.dump_outputs(str(tmp_path / "b"), prod.copy())
    sa, ca = _load(tmp_path / "a")
    sb, cb = _load(tmp_path / "b")
    assert sa.dtype == np.float64 and ca.dtype == np.float64
    assert (sa == sb).all() and (ca == cb).all()
    assert sa.shape[1] == 2 and 2 <= sa.shape[0] <= n
    lo, hi = [int(v) for v in prod & np.uint64(0xffffffff)], [int(v) for v in prod >> np.uint64(32)]
    assert tuple(sa[0]) == (lo[0], hi[0]) and tuple(sa[-1]) == (lo[-1], hi[-1])
    C = bench.DUMP_CHUNK
    assert ca.shape == (4, 2)
    for c in range(4):
        assert int(ca[c, 0]) == sum(lo[c * C:(c + 1) * C]) and int(ca[c, 1]) == sum(hi[c * C:(c + 1) * C])
    # one changed limb anywhere shows in the chunk sums
    prod2 = prod.copy()
    prod2[2 * C + 5] ^= np.uint64(1 << 40)
    bench.dump_outputs(str(tmp_path / "c"), prod2)
    assert (_load(tmp_path / "c")[1] != ca).any()
