"""GPU tests of the device-resident entries on pointers that are only limb-aligned (include/mpfft.h:
operands and results need 8-byte alignment, as the mpn_* calls they replace are handed rp + k).

Every operand and the result start at an odd limb of a larger poisoned allocation (8 mod 16 bytes);
the workspace and the cache stay as allocated.  The result must be limb-equal to the same call on
aligned pointers and to the exact value, and the guard limbs around the result and around every
operand must be unchanged.  One shape per kernel that touches user memory in units wider than a limb:
the fold combine, the fused split of the register column pass (its staged 16-byte loads on an aligned
operand, its guarded limb loads on an odd one: the branch is taken per operand, so the multiply and
the sums also run with one operand odd and the others aligned; which branch ran does not show from
outside, only that both give the same limbs), the small-coefficient kernels and the chains that end
the mod products and the signed sums."""
import numpy as np
import pytest

import stage_model as sm
import sweep_shapes as ss
from helpers import from_int, to_int
from test_gpu_mulmod import full_L
from test_gpu_mulmodm1 import full_L as full_L_m1
from test_gpu_mulmodm1 import modm1
from test_gpu_sdot import torch_dev   # noqa: F401 (a fixture)
from test_mulmodw_cpu import full_Lw

pytestmark = pytest.mark.gpu


def _sync():
    import torch
    torch.cuda.synchronize()


def _both(dev, run, rlen, operands, mixed=False):
    """run(d_r, *operand tensors) on aligned and on odd-limb views -- mixed: also each operand alone
    at an odd limb, the others aligned (the kernels look at each operand's pointer on its own): the
    results (checked equal), every guard intact, every operand unchanged"""
    k = len(operands)
    patterns = [(False,) * (k + 1), (True,) * (k + 1)]
    if mixed:
        patterns += [tuple(j == i for j in range(k)) + (i % 2 == 0,) for i in range(k)]
    out = []
    for pat in patterns:
        ops = [ss.Guarded(dev, len(a), odd, a) for a, odd in zip(operands, pat)]
        dr = ss.Guarded(dev, rlen, pat[k])
        for g, odd in zip(ops + [dr], pat):
            assert g.t.data_ptr() % 16 == (8 if odd else 0)
        run(dr.t, *[g.t for g in ops])
        _sync()
        assert dr.intact(), "guard limbs around d_r changed (odd = %s)" % (pat,)
        for g, a in zip(ops, operands):
            assert g.intact() and (g.host() == a).all(), "an operand or its guard limbs changed (odd = %s)" % (pat,)
        out.append(dr.host())
    for o, pat in zip(out[1:], patterns[1:]):
        assert (out[0] == o).all(), "limb-aligned pointers change the result (odd = %s)" % (pat,)
    return out[1]


MUL_SHAPES = [(5, 4096, 20000, 19000, "k_cmeta + k_combine_red", None), (8, 512, 40000, 40000, None, "k_rpass"),
              (9, 2, 120, 97, None, None)]


@pytest.mark.parametrize("depth,w,n1,n2,combine,columns", MUL_SHAPES, ids=["d%d-w%d-%d-%d" % s[:4] for s in MUL_SHAPES])
def test_mul_and_sqr(mp, oracle, torch_dev, depth, w, n1, n2, combine, columns):
    sk = mp.stage_kernels(n1, n2, depth, w)
    if combine:
        assert sk["combine"].startswith(combine), sk   # the fold combine
    if columns:
        assert sk["fwd_columns"].startswith(columns) and "split" in sk["fwd_columns"], sk   # the fused split
    a, b = mp.fill_random(n1, 0xa11 + depth), mp.fill_random(n2, 0xa12 + depth)
    ws = mp.alloc_workspace(n1, n2, depth, w, torch_dev)
    wsq = mp.alloc_workspace_sqr(n1, depth, w, torch_dev)

    def mul(dr, da, db):
        ws.fill_(0xFF)
        mp.mul_device(dr, da, n1, db, n2, depth, w, ws)

    def sqr(dr, da):
        wsq.fill_(0xFF)
        mp.sqr_device(dr, da, n1, depth, w, wsq)
    assert (_both(torch_dev, mul, n1 + n2, [a, b], mixed=True) == oracle.gmp_mul(a, b)).all()
    assert (_both(torch_dev, sqr, 2 * n1, [a]) == oracle.gmp_mul(a, a)).all()


MOD_SHAPES = [("mulmod", 6, 64, 4088), ("mulmod", 5, 4096, full_L(5, 4096)), ("mulmodm1", 6, 64, 4088),
              ("mulmodm1", 5, 4096, full_L_m1(5, 4096)), ("mulmodw", 6, 64, 4088), ("mulmodw", 5, 4096, full_Lw(5, 4096))]


@pytest.mark.parametrize("family,depth,w,L", MOD_SHAPES, ids=["%s-d%d-w%d-L%d" % s for s in MOD_SHAPES])
def test_mod_products(mp, oracle, torch_dev, family, depth, w, L):
    assert getattr(mp, family + "_check_params")(L, depth, w) == 0
    m1 = family == "mulmodm1"
    nl = L if m1 else L + 1
    a, b = mp.fill_random(nl, 0xa21 + depth), mp.fill_random(nl, 0xa22 + depth)
    if not m1:
        a[L] = b[L] = 0
    stem = family[3:]
    wsm = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev) if m1 else getattr(mp, "alloc_workspace_" + family)(L, depth, w, False, torch_dev)
    wss = mp.alloc_workspace_mulmodm1(L, depth, w, 1, torch_dev) if m1 else getattr(mp, "alloc_workspace_" + family)(L, depth, w, True, torch_dev)

    def mul(dr, da, db):
        wsm.fill_(0xFF)
        getattr(mp, "mul" + stem + "_device")(dr, da, db, L, depth, w, wsm)

    def sqr(dr, da):
        wss.fill_(0xFF)
        getattr(mp, "sqr" + stem + "_device")(dr, da, L, depth, w, wss)
    fold = (lambda v: modm1(v, 64 * L)) if m1 else (lambda v: sm.modp(v, 64 * L))
    # random operands, then the value whose square sends a carry or borrow through every limb of the chain
    edge = from_int((1 << (64 * L)) - 2, nl) if m1 else from_int((1 << (64 * L)) - 1, nl)
    for x, y in ((a, b), (edge, edge)):
        assert to_int(_both(torch_dev, mul, nl, [x, y])) == fold(to_int(oracle.gmp_mul(x, y))), family
        assert to_int(_both(torch_dev, sqr, nl, [x])) == fold(to_int(oracle.gmp_mul(x, x))), family


def test_cached_operand(mp, oracle, torch_dev):
    """d_i2 of precomp_device and d_i1 of mul_precomp_device both offset; the cache as allocated"""
    depth, w, n = 5, 4096, 20000
    a, b = mp.fill_random(n, 0xa31), mp.fill_random(n, 0xa32)
    wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
    wsp = mp.alloc_workspace_mul_precomp(n, n, depth, w, torch_dev)
    caches = []
    for odd in (False, True):
        gb = ss.Guarded(torch_dev, n, odd, b)
        pre = mp.alloc_precomp(n, n, depth, w, torch_dev)
        pre.fill_(0x5A)
        wsm.fill_(0xFF)
        mp.precomp_device(pre, gb.t, n, n, depth, w, wsm)
        _sync()
        assert gb.intact() and (gb.host() == b).all()
        caches.append(pre)
    assert bool((caches[0] == caches[1]).all()), "a limb-aligned operand changes the cache"

    def run(dr, da):
        wsp.fill_(0xFF)
        mp.mul_precomp_device(dr, da, n, caches[1], n, depth, w, wsp)
    assert (_both(torch_dev, run, 2 * n, [a]) == oracle.gmp_mul(a, b)).all()


@pytest.mark.parametrize("depth,w,n", [(5, 4096, 20000), (11, 8, 5000)])
def test_sums_and_signed_sums(mp, oracle, torch_dev, depth, w, n):
    K, neg = 3, 0b101
    assert mp.sdot_check_params(K, neg, n, n, depth, w) == 0
    ha = [mp.fill_random(n, 0xa41 + i) for i in range(K)]
    hb = [mp.fill_random(n, 0xa51 + i) for i in range(K)]
    prods = [to_int(oracle.gmp_mul(x, y)) for x, y in zip(ha, hb)]
    wsd = mp.alloc_workspace_dot(K, n, n, depth, w, torch_dev)
    wss = mp.alloc_workspace_sdot(K, n, n, depth, w, torch_dev)

    def dot(dr, *ops):
        wsd.fill_(0xFF)
        mp.dot_device(dr, list(ops[:K]), list(ops[K:]), n, n, depth, w, wsd)

    def sdot(dr, *ops):
        wss.fill_(0xFF)
        mp.sdot_device(dr, list(ops[:K]), list(ops[K:]), neg, n, n, depth, w, wss)
    nl = 2 * n + 1
    assert (_both(torch_dev, dot, nl, ha + hb, mixed=True) == from_int(sum(prods), nl)).all()
    val = sum((-1 if (neg >> i) & 1 else 1) * p for i, p in enumerate(prods))
    got = _both(torch_dev, sdot, nl, ha + hb)
    assert (got == from_int(val % (1 << (64 * nl)), nl)).all() and mp.sdot_to_int(got) == val
