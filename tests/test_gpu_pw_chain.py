"""GPU tests of the carry chains around k_pwss's inner product (pkernels.hpp: pw_canon's common
path on the low word and its two folds, pw_sqrt2's four interleaved chains and its rippled carry),
one per kernel family: the smallest l = 1024 (M = 10), 2048 (M = 18) and 4096 (M = 20) shapes of
stage_model.TABLE.

The pointwise stage alone (mpfft_stage, as tests/test_gpu_pw_kara.py drives it: the stage entry
runs the FUSE 0 form) on hand-placed residues, every pair of the patterns below, against exact
Python-int products mod 2^N + 1.  A value with one non-zero piece v at piece t0 transforms to
v theta^(t0 (2k+1)) in every inner slot k: the limbs stay v (rotations are pending exponents), so
the pieces' low words are what pw_canon meets, give or take the top that pw_norm moved into them:
  * piece 0 with low word 0, with low word 0xffffffff, and the value 1 (pw_canon's wrapped low
    word in both directions, and its common path next to it);
  * 2^N exactly (limbs 0, carry limb 1: piece 0 is -1, a borrow through every word);
  * an odd piece (half-integer weight: pw_sqrt2) that is all ones, and the top piece with low word
    0xffffffff (the low half's carry meets a high half of zeros / ones);
  * all-ones and zero operands; random.
Then one whole product per shape through the form the planner picks there, and through the pair
and quad forms of l = 2048 on sparse operands (single-bit limbs: every slot's pieces are 0 or a
power of two), against the exact product."""
import os
import random

import numpy as np
import pytest

import stage_model as SM
from helpers import max_limbs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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


def _row(l):
    """the smallest shape of stage_model.TABLE with l limbs per coefficient"""
    rows = [r for r in SM.TABLE if r["l"] == l]
    return min(rows, key=lambda r: (r["depth"], SM.table_n(r)))


# (l, MPFFT_POINTWISE, kernel, K): l = 1024 takes k_pwss only when asked to (k_pwm2 is faster there)
SHAPES = [(1024, "pwss", "k_pwss<10", 256), (2048, None, "k_pwss<18", 256), (4096, None, "k_pwss<20", 512)]
NK = 9


def _pattern(kind, l, N, K, rng):
    """canonical residue (limbs value, carry limb)"""
    B = N // K                                                   # bits per piece
    r = rng.getrandbits(B - 40) | 1
    if kind == 1:
        return 0, 1                                              # 2^N == -1
    v = {0: rng.getrandbits(N), 2: (1 << N) - 1, 3: 0,
         4: r << 32,                                             # piece 0, low word 0
         5: r << 32 | 0xffffffff,                                # piece 0, low word 0xffffffff
         6: 1,
         7: ((1 << B) - 1) << B,                                 # piece 1 (odd: pw_sqrt2) all ones
         8: (r << 32 | 0xffffffff) << (B * (K - 1))}[kind]       # the top piece, low word 0xffffffff
    return v, 0


@pytest.mark.parametrize("l,kind,head,K", SHAPES)
def test_pointwise_stage_on_placed_chain_values(mp, torch_dev, l, kind, head, K):
    import torch
    from gpu_stages import _cbs, _val_reduced
    row = _row(l)
    depth, w, n1 = row["depth"], row["w"], SM.table_n(row)
    n2 = n1
    P = mp.plan_info(n1, n2, depth, w)
    T, N = P["trunc"], P["n"] * w
    assert P["l"] == l and N == 64 * l
    assert T >= NK * NK   # every pair of patterns is placed
    p = (1 << N) + 1
    rng = random.Random(1009 * depth + w)
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n1, n2, depth, w)["pointwise"]
        assert ran.startswith(head) and "K=%d" % K in ran, ran
        ws = mp.alloc_workspace(n1, n2, depth, w, torch_dev)
        ws.fill_(0)
        digA, topA, digB, topB = mp.workspace_views(ws, n1, n2, depth, w)
        want = []
        host = {k: (np.zeros((T, l), np.uint64), np.zeros(T, np.int32)) for k in "AB"}
        for sl in range(T):
            va, ta = _pattern(sl % NK, l, N, K, rng)
            vb, tb = _pattern((sl // NK) % NK, l, N, K, rng)
            for k, v, t in (("A", va, ta), ("B", vb, tb)):
                host[k][0][sl] = np.frombuffer(v.to_bytes(8 * l, "little"), dtype=np.uint64)
                host[k][1][sl] = t
            want.append((va + ta * (1 << N)) * (vb + tb * (1 << N)) % p)
        for k, dig, top in (("A", digA, topA), ("B", digB, topB)):
            dig[:T] = torch.from_numpy(host[k][0].view(np.int64)).to(torch_dev)
            top[:T] = torch.from_numpy(host[k][1]).to(torch_dev)
        da = torch.zeros(n1, dtype=torch.int64, device=torch_dev)
        db = torch.zeros(n2, dtype=torch.int64, device=torch_dev)
        dr = torch.zeros(n1 + n2, dtype=torch.int64, device=torch_dev)
        mp.stage(mp.STAGE_POINTWISE, da, db, dr, n1, n2, depth, w, ws)
        torch.cuda.synchronize()
    dig = digA.cpu().numpy().view(np.uint64)
    top = topA.cpu().numpy().astype(np.int64)
    cb = _cbs(mp, ws, n1, n2, depth, w, 0)
    bad = [sl for sl in range(T) if _val_reduced(dig, top, cb, sl, N) % p != want[sl]]
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]} (patterns A = slot % {NK}, B = slot // {NK} % {NK})"


def _sparse(n, rng):
    """single-bit limbs: bit 0 of limb 0, bit 63 of the top limb, a few more"""
    a = np.zeros(n, np.uint64)
    a[0] = 1
    a[n - 1] = 1 << 63
    for _ in range(5):
        a[rng.randrange(n)] = 1 << rng.randrange(64)
    return a


@pytest.mark.parametrize("l,kind,head,K", SHAPES)
def test_whole_product_at_the_table_shapes(mp, oracle, torch_dev, l, kind, head, K):
    row = _row(l)
    depth, w, n = row["depth"], row["w"], SM.table_n(row)
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n, n, depth, w)["pointwise"]
        assert ran.startswith(head), ran
        a, b = mp.fill_random(n, 0xc400 + depth), mp.fill_random(n, 0xc500 + w)
        assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), (depth, w, ran)


PAIR, QUAD = "pair + last row level", "quad + last two row levels"


@pytest.mark.parametrize("depth,w,n,fused", [(8, 512, 40000, PAIR), (14, 8, 500000, QUAD)])
def test_fused_forms_on_sparse_operands(mp, oracle, torch_dev, depth, w, n, fused):
    ran = mp.stage_kernels(n, n - 17, depth, w)["pointwise"]
    assert ran.startswith("k_pwss<18") and fused in ran, ran
    rng = random.Random(depth)
    a, b = _sparse(n, rng), mp.fill_random(n - 17, 0xc600 + w)
    assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), ("sparse x random", depth, w, ran)
    b = _sparse(n - 17, rng)
    assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), ("sparse x sparse", depth, w, ran)
