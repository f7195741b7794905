"""Shape enumerators shared by tests/test_sweep_shapes_cpu.py and the GPU sweeps
(tests/test_gpu_sweep_mod.py, tests/test_gpu_sweep_mul.py).

The curated tables of the per-family GPU modules hold one shape per pointwise family and combine
path; the planners accept far more.  The grids here run every (depth, w) of DEPTHS x WS at its
largest valid size, kept when that size is at most `cap` limbs, so that one product stays a few
milliseconds.  No GPU is needed to enumerate: the planners run on the host."""
from helpers import max_limbs

DEPTHS = tuple(range(2, 16))
WS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048, 4096)
MOD_FAMILIES = ("mulmod", "mulmodm1", "mulmodw")
MAX_L = 4096   # limbs per coefficient the kernels are built for


def mod_bits1(family, depth, w):
    """the largest bits1 of the family's bound at (depth, w), before the multiple-of-64 condition"""
    N = (1 << depth) * w
    return {"mulmod": (N - depth - 2) // 2, "mulmodm1": (N - depth - 1) // 2, "mulmodw": (N + 32 - depth - 2) // 2}[family]


def mod_full_L(family, depth, w):
    """the largest L of (depth, w): the largest bits1 within the family's bound with 2n bits1 a
    multiple of 64 (0 when there is none; mulmodw needs bits1 >= 32)"""
    n = 1 << depth
    b = mod_bits1(family, depth, w)
    while b > 0 and (2 * n * b) % 64:
        b -= 1
    if b <= 0 or (family == "mulmodw" and b < 32):
        return 0
    return 2 * n * b // 64


def mod_grid(family, cap=20000):
    """[(depth, w, L)]: every (depth, w) of the grid with 64 | N and N / 64 <= 4096 at its largest L,
    kept when 1 <= L <= cap"""
    out = []
    for depth in DEPTHS:
        for w in WS:
            N = (1 << depth) * w
            if N % 64 or N // 64 > MAX_L:
                continue
            L = mod_full_L(family, depth, w)
            if 1 <= L <= cap:
                out.append((depth, w, L))
    return out


def mod_deep(family):
    """depth 11..14 x w in {1, 2, 3, 4} at L = 18944: NC up to 128 and NR up to 256, several passes
    each way on coefficients of 32 to 1024 limbs, bits1 from 296 down to 37"""
    out = []
    for depth in (11, 12, 13, 14):
        step = 1 << (depth - 5)
        for w in (1, 2, 3, 4):
            out.append((depth, w, 19000 // step * step))
    return out


def mod_edges(family):
    """result lengths on and around a block edge of the chains that end the products (k_nwrap and
    k_nwrapw: 1024-limb blocks, k_cwrap: 2048-limb blocks), pieces of 1, 2 and 3 bits, mulmodw's
    bits1 >= 32 edge and its power-of-two B"""
    if family == "mulmodm1":
        out = [(5, 256, L) for L in (2047, 2048, 2049)] + [(5, 512, L) for L in (4095, 4096, 4097, 6143, 6144, 6145)]
    else:
        out = [(5, 128, L) for L in (1023, 1024, 1025)] + [(5, 256, L) for L in (2047, 2048, 2049, 3071, 3072, 3073)]
    if family == "mulmodw":
        out += [(5, 128, 2048), (5, 256, 4096), (5, 64, 32), (5, 64, 33)]
    else:
        out += [(5, 4096, L) for L in (1, 2, 3)]
    return out


def mul_limbs(K, depth, w):
    """the largest balanced n1 = n2 of a K-term sum at (depth, w); K = 1: the multiply's own bound"""
    if K == 1:
        return max_limbs(depth, w)
    N = (1 << depth) * w
    bits1 = (N - depth - (K - 1).bit_length()) // 2
    return (1 << depth) * bits1 // 64


def mul_grid(K, cap=20000):
    """[(depth, w, n)]: the same (depth, w) grid at the largest balanced n of a K-term sum, kept when
    1 <= n <= cap (K = 1 serves the square and the cached operand).  Arithmetic only, as mod_grid:
    tests/test_sweep_shapes_cpu.py checks every shape against dot_check_params and dot_max_limbs."""
    out = []
    for depth in DEPTHS:
        for w in WS:
            N = (1 << depth) * w
            if N % 64 or N // 64 > MAX_L:
                continue
            n = mul_limbs(K, depth, w)
            if 1 <= n <= cap:
                out.append((depth, w, n))
    return out


GUARD = 64                      # poisoned limbs on both sides of a guarded device array
POISON = 0x6b6b6b6b6b6b6b6b


class Guarded:
    """n limbs on the device between two runs of GUARD poisoned limbs; .t is the view to hand to the
    library.  odd: the view starts at an odd limb of the allocation (8 mod 16 bytes), as rp + k does."""

    def __init__(self, dev, n, odd=False, data=None):
        import numpy as np
        import torch
        self.lo = GUARD + (1 if odd else 0)
        self.buf = torch.full((self.lo + n + GUARD,), POISON, dtype=torch.int64, device=dev)
        self.t = self.buf[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == (8 if odd else 0)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint64).view(np.int64)))

    def intact(self):
        n = self.t.numel()
        return bool((self.buf[:self.lo] == POISON).all()) and bool((self.buf[self.lo + n:] == POISON).all())

    def host(self):
        import numpy as np
        return self.t.cpu().numpy().view(np.uint64)


def by_depth(shapes):
    """{depth: [shape]} in grid order"""
    out = {}
    for s in shapes:
        out.setdefault(s[0], []).append(s)
    return out


def stage_kernels(mp, family, shape):
    """the stage -> kernel dict and the plan of `shape` in `family`: a mod family, "mul", "sqr" or
    "dot<K>" (shape = (depth, w, n) with n1 = n2 = n)"""
    depth, w, n = shape
    if family in MOD_FAMILIES:
        return getattr(mp, family + "_stage_kernels")(n, depth, w), getattr(mp, family + "_plan_info")(n, depth, w)
    if family == "mul":
        return mp.stage_kernels(n, n, depth, w), mp.plan_info(n, n, depth, w)
    if family == "sqr":
        return mp.sqr_stage_kernels(n, depth, w), mp.plan_info(n, n, depth, w)
    assert family.startswith("dot"), family
    K = int(family[3:])
    return mp.dot_stage_kernels(K, n, n, depth, w), mp.dot_plan_info(K, n, n, depth, w)


def signature(mp, family, shape):
    """what tells two plans apart: the stage-kernel strings (whitespace-normalised), l, NC, NR and
    the parity of w"""
    sk, P = stage_kernels(mp, family, shape)
    return tuple(" ".join(sk[k].split()) for k in sorted(sk)) + (P["l"], P["NC"], P["NR"], shape[1] % 2)
