"""GPU tests of k_pwss's inner product (pw_mulmod: Karatsuba over the N'/2 halves where
pw_kara<M>() ships it, schoolbook elsewhere), one per kernel family l = 1024 (M = 10), 2048
(M = 18) and 4096 (M = 20).

The pointwise stage alone (mpfft_stage, FUSE 0: the stage entry never fuses row levels) on
hand-placed residues, every pair of: 0, 1, 2^N (the carry limb), 2^N - 1 (all-ones limbs), a
value with only its top piece set, a value with only its lowest piece set, 0x80 bytes, random --
against exact Python-int products mod 2^N + 1.  The fused forms (FUSE 1: slot pairs, FUSE 2: slot
quads) exist only inside a whole multiply, so they are checked as whole products of the smallest
shapes that select them, against GMP.  Every test first asserts the kernel that runs through
mpfft_stage_kernels."""
import os
import random

import numpy as np
import pytest

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


NK = 8


def _pattern(kind, l, N, rng):
    """canonical residue (limbs value, carry limb)"""
    if kind == 1:
        return 0, 1                                              # 2^N == -1
    v = {0: rng.getrandbits(N), 2: (1 << N) - 1, 3: 0, 4: 1,
         5: (rng.getrandbits(64) | 1) << (N - 64),               # only the top piece
         6: rng.getrandbits(64) | 1,                             # only the lowest piece
         7: int.from_bytes(b"\x80" * (8 * l), "little")}[kind]
    return v, 0


@pytest.mark.parametrize("depth,w,kind,head", [(6, 1024, "pwss", "k_pwss<10"), (5, 4096, None, "k_pwss<18"),
                                               (6, 4096, None, "k_pwss<20")])
def test_pointwise_stage_on_placed_values(mp, torch_dev, depth, w, kind, head):
    import torch
    from gpu_stages import _cbs, _val_reduced
    n1 = n2 = max_limbs(depth, w)
    P = mp.plan_info(n1, n2, depth, w)
    l, T, N = P["l"], P["trunc"], P["n"] * w
    assert l == {10: 1024, 18: 2048, 20: 4096}[int(head[-2:])]
    assert T >= NK * NK   # every pair of patterns is placed
    p = (1 << N) + 1
    rng = random.Random(977 * depth + w)
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n1, n2, depth, w)["pointwise"]
        assert ran.startswith(head), ran   # (a whole multiply's kernel: the stage entry runs its FUSE 0 form)
        ws = mp.alloc_workspace(n1, n2, depth, w, torch_dev)
        ws.fill_(0)
        digA, topA, digB, topB = mp.workspace_views(ws, n1, n2, depth, w)
        want = []
        host = {k: (np.zeros((T, l), np.uint64), np.zeros(T, np.int32)) for k in "AB"}
        for sl in range(T):
            va, ta = _pattern(sl % NK, l, N, rng)
            vb, tb = _pattern((sl // NK) % NK, l, N, rng)
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
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]}"


PAIR, QUAD = "pair + last row level", "quad + last two row levels"


@pytest.mark.parametrize("depth,w,n,kind,head,fused", [
    (8, 256, 60000, "pwss", "k_pwss<10", PAIR),
    (8, 512, 40000, None, "k_pwss<18", PAIR),
    (14, 8, 500000, None, "k_pwss<18", QUAD),
    (6, 4096, 131064, None, "k_pwss<20", PAIR),
    (16, 4, 500000, None, "k_pwss<20", QUAD),
])
def test_fused_pointwise_whole_products(mp, oracle, depth, w, n, kind, head, fused):
    with _pointwise_env(kind):
        ran = mp.stage_kernels(n, n - 17, depth, w)["pointwise"]
        assert ran.startswith(head) and fused in ran, ran
        a = mp.fill_random(n, 0x9a00 + depth)
        b = mp.fill_random(n - 17, 0x9b00 + w)
        assert (mp.mul(a, b, depth, w) == oracle.gmp_mul(a, b)).all(), (depth, w, ran)
        o1, o2 = np.full(n, 2**64 - 1, dtype=np.uint64), np.full(n - 17, 2**64 - 1, dtype=np.uint64)
        assert (mp.mul(o1, o2, depth, w) == oracle.gmp_mul(o1, o2)).all(), ("all ones", depth, w, ran)
