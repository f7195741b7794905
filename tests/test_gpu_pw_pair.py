"""GPU tests of the grouped wrap selects in the exchange levels of k_pwss / k_pwsq (pkernels.hpp:
pw_combine GRP and the extra exchange rows 2M .. = ~rows 0 .. of the K = 256 kernels).

The pointwise stage alone (mpfft_stage / mpfft_sqr_stage: FUSE 0, the stage entry never fuses row
levels) on hand-placed residues for k_pwss<10,8,0>, k_pwss<18,8,0>, k_pwsq<10,8,0> and
k_pwsq<18,8,0>, against exact Python integers mod 2^N + 1.  The placed values: 0; 2^N (== -1, the
carry limb); 2^N - 1 (which is also "every piece = 2^B - 1": all-ones limbs); every piece's low
32-bit word 0 with the next word all ones, and the reverse (a reader that takes row 0 plain where
it should take it complemented, or the other way round, differs on these in every piece); two
random residues -- every ordered pair of them for the products, each of them for the squares.

The fused forms (FUSE 1: slot pairs, FUSE 2: slot quads) exist only inside a whole multiply, so
k_pwss<18,8,1>, k_pwss<18,8,2>, k_pwsq<18,8,1> and k_pwsq<18,8,2> are checked as whole products of
the small shapes that select them, against GMP, on random limbs and on limbs of the two word
patterns; the FUSE 0 instances get one whole product each as well.  Every test first asserts the
kernel that runs."""
import os
import random

import numpy as np
import pytest

from helpers import max_limbs

pytestmark = pytest.mark.gpu

PAIR, QUAD = "pair + last row level", "quad + last two row levels"
NV = 7   # placed values per operand


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


def _values(l, N, seed):
    """the NV placed residues as (limbs value, carry limb)"""
    rng = random.Random(seed)
    K = 256
    B = N // K                      # bits per piece (k_pwss cuts a residue into K = 256 pieces)
    assert B * K == N and B >= 64

    def pieces(lo, hi):             # low word lo, next word hi, the rest of each piece random
        v = 0
        for t in range(K):
            v |= (((rng.getrandbits(B - 64) << 64) | (hi << 32) | lo)) << (B * t)
        return v
    return [(0, 0), (0, 1), ((1 << N) - 1, 0), (pieces(0, 0xffffffff), 0), (pieces(0xffffffff, 0), 0),
            (rng.getrandbits(N), 0), (rng.getrandbits(N), 0)]


def _modp(x, N):
    """x mod 2^N + 1 for 0 <= x < 2^(3N) by folding (2^N == -1)"""
    m = (1 << N) - 1
    return ((x & m) - ((x >> N) & m) + (x >> (2 * N))) % (m + 2)


def _limbs(v, l):
    return np.frombuffer(v.to_bytes(8 * l, "little"), dtype=np.uint64)


@pytest.mark.parametrize("depth,w,kind,head,l_want", [(6, 1024, "pwss", "k_pwss<10", 1024), (5, 4096, None, "k_pwss<18", 2048)])
def test_product_stage_on_placed_values(mp, torch_dev, depth, w, kind, head, l_want):
    import torch
    from gpu_stages import _cbs, _val_reduced
    n1 = n2 = max_limbs(depth, w)
    P = mp.plan_info(n1, n2, depth, w)
    l, T, N = P["l"], P["trunc"], P["n"] * w
    assert l == l_want and T >= NV * NV   # every ordered pair is placed
    p = (1 << N) + 1
    vals = _values(l, N, 31 * depth + w)
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n1, n2, depth, w)["pointwise"]
        assert ran.startswith(head), ran
        ws = mp.alloc_workspace(n1, n2, depth, w, torch_dev)
        ws.fill_(0)
        digA, topA, digB, topB = mp.workspace_views(ws, n1, n2, depth, w)
        host = {k: (np.zeros((T, l), np.uint64), np.zeros(T, np.int32)) for k in "AB"}
        want = []
        for sl in range(T):
            (va, ta), (vb, tb) = vals[sl % NV], vals[(sl // NV) % NV]
            host["A"][0][sl], host["A"][1][sl] = _limbs(va, l), ta
            host["B"][0][sl], host["B"][1][sl] = _limbs(vb, l), tb
            want.append(_modp((va + ta * (1 << N)) * (vb + tb * (1 << N)), N))
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
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]} (value kinds A = slot % {NV}, B = slot // {NV} % {NV})"


@pytest.mark.parametrize("depth,w,kind,head,l_want", [(6, 1024, "pwss", "k_pwsq<10>", 1024), (5, 4096, None, "k_pwsq<18>", 2048)])
def test_square_stage_on_placed_values(mp, torch_dev, depth, w, kind, head, l_want):
    import torch
    from gpu_stages import _val_reduced
    n = max_limbs(depth, w)
    P = mp.plan_info(n, n, depth, w)
    l, T, N = P["l"], P["trunc"], P["n"] * w
    assert l == l_want and T >= NV
    p = (1 << N) + 1
    vals = _values(l, N, 37 * depth + w)
    with _pointwise_env(kind):
        ran = mp.sqr_stage_kernels(n, depth, w)["pointwise"]
        assert ran.startswith(head), ran
        ws = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
        ws.fill_(0)
        digA, topA = mp.sqr_workspace_views(ws, n, depth, w)
        hd, ht = np.zeros((T, l), np.uint64), np.zeros(T, np.int32)
        want = []
        for sl in range(T):
            v, t = vals[sl % NV]
            hd[sl], ht[sl] = _limbs(v, l), t
            want.append(_modp((v + t * (1 << N)) ** 2, N))
        digA[:T] = torch.from_numpy(hd.view(np.int64)).to(torch_dev)
        topA[:T] = torch.from_numpy(ht).to(torch_dev)
        da = torch.zeros(n, dtype=torch.int64, device=torch_dev)
        dr = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
        mp.sqr_stage(mp.STAGE_POINTWISE, da, dr, n, depth, w, ws)
        torch.cuda.synchronize()
    lay = mp.sqr_workspace_layout(n, depth, w)
    slots, cbw = lay["slots"], lay["cbw"]
    cb = ws.view(torch.uint8)[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
    cb = cb.cpu().numpy().view(np.uint64)
    dig = digA.cpu().numpy().view(np.uint64)
    top = topA.cpu().numpy().astype(np.int64)
    bad = [sl for sl in range(T) if _val_reduced(dig, top, cb, sl, N) % p != want[sl]]
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]} (value kind = slot % {NV})"


def _operands(mp, n, seed):
    """random limbs; every limb low word 0, high word all ones; the reverse"""
    return [mp.fill_random(n, seed), np.full(n, 0xffffffff00000000, dtype=np.uint64),
            np.full(n, 0x00000000ffffffff, dtype=np.uint64)]


WHOLE = [
    (6, 1024, 32760, "pwss", "10", None),
    (5, 4096, 20000, None, "18", None),
    (8, 512, 40000, None, "18", PAIR),
    (14, 8, 500000, None, "18", QUAD),
]


@pytest.mark.parametrize("depth,w,n,kind,M,fused", WHOLE)
def test_whole_products(mp, oracle, depth, w, n, kind, M, fused):
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n, n - 17, depth, w)["pointwise"]
        assert ran.startswith("k_pwss<" + M), ran
        assert (fused in ran) if fused else ("pair" not in ran and "quad" not in ran), ran
        for a, b in zip(_operands(mp, n, 0x7a00 + depth), _operands(mp, n - 17, 0x7b00 + w)[::-1]):
            assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), (depth, w, ran)


@pytest.mark.parametrize("depth,w,n,kind,M,fused", WHOLE)
def test_whole_squares(mp, oracle, depth, w, n, kind, M, fused):
    with _pointwise_env(kind):
        ran = mp.sqr_stage_kernels(n, depth, w)["pointwise"]
        assert ran.startswith("k_pwsq<" + M), ran
        assert (fused in ran) if fused else ("pair" not in ran and "quad" not in ran), ran
        for a in _operands(mp, n, 0x7c00 + depth):
            assert (mp.sqr(a, depth, w) == oracle.gmp_mul(a, a)).all(), (depth, w, ran)
