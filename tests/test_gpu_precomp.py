"""GPU tests of multiplication by a precomputed operand (mpfft_precomp_*, mpfft_mul_precomp_*): whole
products through every pointwise class (k_pwsx / k_pwsp<10/18/20> at FUSE 0, 1, 2, and the other
families reading B from the cache), the two kernels alone on hand-placed residues, equality with
the multiply, the workspace and cache bounds, a cache shared by two streams, back-to-back calls,
profiling, the host handle and a plain C caller.  The reference is GMP (oracle.gmp_mul) or exact
integer arithmetic; bit-exact is the only bar.  Every test asserts the kernel class of its shape
through precomp_stage_kernels first, so a planner change cannot silently move it."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import max_limbs
from test_gpu_sqr import FOLD, PAIR, QUAD, _modp, _pattern, _pointwise_env, _val_reduced

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENOMEM, EINVAL = 4, 1


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _check_class(mp, n1, n2, depth, w, head, has=(), whole=True):
    """head: 'k_pwsp<M>' (the cache is then written by k_pwsx<M> with the same suffix), or the
    family that reads B's row arrays from the cache"""
    sk = mp.precomp_stage_kernels(n1, n2, depth, w)
    pw, pre = sk["pointwise"], sk["precomp"]
    assert pw.startswith(head), (depth, w, n1, n2, pw)
    for s in has:
        assert s in pw and s in pre, (depth, w, n1, n2, pw, pre)
    if head.startswith("k_pwsp"):
        assert pre == pw.replace("k_pwsp", "k_pwsx"), (pw, pre)
        if whole and not has:
            assert "pair" not in pw and "quad" not in pw, pw   # FUSE 0
    else:
        assert pw.endswith("(B cached)") and pre == "copy", (pw, pre)
    return sk


def _dev(torch, dev, a):
    return torch.from_numpy(a.view(np.int64)).to(dev)


class _Cached:
    """operand b cached on the device for products with n1-limb operands"""

    def __init__(self, mp, dev, b, n1, depth, w, wsm=None):
        import torch
        self.mp, self.dev, self.n1, self.n2, self.depth, self.w = mp, dev, n1, len(b), depth, w
        self.pre = mp.alloc_precomp(n1, self.n2, depth, w, dev)
        wsm = wsm if wsm is not None else mp.alloc_workspace(n1, self.n2, depth, w, dev)
        mp.precomp_device(self.pre, _dev(torch, dev, b), n1, self.n2, depth, w, wsm)
        torch.cuda.synchronize()
        self.ws = mp.alloc_workspace_mul_precomp(n1, self.n2, depth, w, dev)

    def mul(self, a):
        import torch
        dr = torch.zeros(self.n1 + self.n2, dtype=torch.int64, device=self.dev)
        self.mp.mul_precomp_device(dr, _dev(torch, self.dev, a), self.n1, self.pre, self.n2, self.depth, self.w, self.ws)
        torch.cuda.synchronize()
        return dr.cpu().numpy().view(np.uint64)


# (depth, w, n, MPFFT_POINTWISE, pointwise starts with, pointwise contains, scale, combine)
# the nested shapes are those of test_gpu_sqr.py::WHOLE, the smallest that reach each instance
WHOLE = [
    (7, 1024, 131064, None, "k_pwsp<18>", (), "k_rscale", "k_combine1"),
    (5, 4096, 20000, None, "k_pwsp<18>", (), "(folded", FOLD),
    (8, 512, 40000, None, "k_pwsp<18>", (PAIR,), None, None),
    (8, 512, 140000, None, "k_pwsp<18>", (PAIR,), None, None),
    (14, 8, 500000, None, "k_pwsp<18>", (QUAD,), None, None),
    (12, 64, 500000, None, "k_pwsp<20>", (), None, None),
    (6, 4096, 131064, None, "k_pwsp<20>", (PAIR,), None, None),
    (16, 4, 500000, None, "k_pwsp<20>", (QUAD,), None, None),
    (6, 1024, 32760, "pwss", "k_pwsp<10>", (), None, None),
    (9, 2, 120, None, "k_pointwise", (), None, None),
    (11, 8, 5000, None, "k_pwm2", (), None, None),
    (9, 16, None, None, "k_pwm ", (), None, None),     # l = 128, n = max_limbs
    (8, 8, None, None, "k_pw ", (), None, None),       # l = 32, n = max_limbs
]


@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine", WHOLE)
def test_whole_products_every_pointwise_class(mp, oracle, torch_dev, depth, w, n, kind, head, has, scale, combine):
    """mul_precomp_device(a, precomp_device(b)) against GMP: a random and an all-ones cached operand,
    the random one's cache reused for three different a."""
    if n is None:
        n = max_limbs(depth, w)
    with _pointwise_env(kind):
        sk = _check_class(mp, n, n, depth, w, head, has)
        if scale:
            assert sk["scale"].startswith(scale), sk["scale"]
        if combine:
            assert sk["combine"].startswith(combine), sk["combine"]
        if (depth, w, n) == (8, 512, 140000):   # case b
            P = mp.plan_info(n, n, depth, w)
            assert P["trunc"] > P["n"]
        wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
        ones = np.full(n, 2**64 - 1, dtype=np.uint64)
        b = mp.fill_random(n, 0x6000 + 31 * depth + w)
        cb = _Cached(mp, torch_dev, b, n, depth, w, wsm)
        for a in (mp.fill_random(n, 0x6100 + w), mp.fill_random(n, 0x6200 + depth), ones):
            assert (cb.mul(a) == oracle.gmp_mul(a, b)).all(), (depth, w, n, sk["pointwise"])
        co = _Cached(mp, torch_dev, ones, n, depth, w, wsm)
        for a in (ones, b):
            assert (co.mul(a) == oracle.gmp_mul(a, ones)).all(), (depth, w, n, sk["pointwise"])


@pytest.mark.parametrize("n1,n2", [(200000, 60000), (60000, 200000)])
def test_unbalanced_operands(mp, oracle, torch_dev, n1, n2):
    """The cached operand's zero bound (its own operand's, zero_op[1]) and the truncation (both
    operands') come from different operands."""
    depth, w = 8, 512
    _check_class(mp, n1, n2, depth, w, "k_pwsp<18>", (PAIR,))
    b = mp.fill_random(n2, 0x7001 + n2)
    cb = _Cached(mp, torch_dev, b, n1, depth, w)
    for a in (mp.fill_random(n1, 0x7002 + n1), np.full(n1, 2**64 - 1, dtype=np.uint64)):
        assert (cb.mul(a) == oracle.gmp_mul(a, b)).all(), (n1, n2)


@pytest.mark.parametrize("depth,w,kind,head", [(5, 4096, None, "k_pwsp<18>"), (6, 4096, None, "k_pwsp<20>"),
                                               (6, 1024, "pwss", "k_pwsp<10>"), (9, 16, None, "k_pwm ")])
def test_store_and_pointwise_stages_on_placed_values(mp, torch_dev, depth, w, kind, head):
    """k_pwsx and k_pwsp alone (the copy and the cache-reading k_pwm on the last shape): B's eight
    patterns placed in B's row arrays of the multiply's workspace -> precomp_stage(PRE_STORE); A's
    patterns in the workspace without B's arrays, shifted by slot / 8 so that every ordered pair of
    patterns meets (2^N x 2^N included) -> mul_precomp_stage(POINTWISE); every live slot's value
    against a b mod 2^N + 1."""
    import torch
    n = max_limbs(depth, w)
    P = mp.plan_info(n, n, depth, w)
    l, T, N = P["l"], P["trunc"], P["n"] * w
    p = (1 << N) + 1
    assert T >= 64   # all 64 ordered pairs of patterns occur
    rng = random.Random(depth * 1000 + w + 7)
    with _pointwise_env(kind):
        _check_class(mp, n, n, depth, w, head, whole=False)   # (the stage entries never fuse row levels)
        wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
        wsm.fill_(0)
        _, _, digB, topB = mp.workspace_views(wsm, n, n, depth, w)
        hb, tb = np.zeros((T, l), np.uint64), np.zeros(T, np.int32)
        ha, ta = np.zeros((T, l), np.uint64), np.zeros(T, np.int32)
        want, pairs = [], set()
        for sl in range(T):
            kb, ka = sl % 8, (sl + sl // 8) % 8
            pairs.add((ka, kb))
            vb, t2 = _pattern(kb, l, N, rng)
            va, t1 = _pattern(ka, l, N, rng)
            hb[sl] = np.frombuffer(vb.to_bytes(8 * l, "little"), dtype=np.uint64)
            ha[sl] = np.frombuffer(va.to_bytes(8 * l, "little"), dtype=np.uint64)
            tb[sl], ta[sl] = t2, t1
            want.append(_modp((va + t1 * (1 << N)) * (vb + t2 * (1 << N)), N))
        assert len(pairs) == 64
        digB[:T] = torch.from_numpy(hb.view(np.int64)).to(torch_dev)
        topB[:T] = torch.from_numpy(tb).to(torch_dev)
        pre = mp.alloc_precomp(n, n, depth, w, torch_dev)
        mp.precomp_stage(mp.STAGE_PRE_STORE, pre, None, n, n, depth, w, wsm)
        torch.cuda.synchronize()
        del wsm
        # the multiply's workspace without B's arrays: A's arrays sit where the multiply's do
        lay = mp.workspace_layout(n, n, depth, w)
        slots, cbw = lay["slots"], lay["cbw"]
        ws = mp.alloc_workspace_mul_precomp(n, n, depth, w, torch_dev)
        ws.fill_(0)
        u8 = ws.view(torch.uint8)
        digA = u8[lay["digA"]:lay["digA"] + slots * l * 8].view(torch.int64).view(slots, l)
        topA = u8[lay["topA"]:lay["topA"] + slots * 4].view(torch.int32)
        cbA = u8[lay["cbA"]:lay["cbA"] + slots * cbw * 8].view(torch.int64).view(slots, cbw)
        digA[:T] = torch.from_numpy(ha.view(np.int64)).to(torch_dev)
        topA[:T] = torch.from_numpy(ta).to(torch_dev)
        keep = pre.clone()
        mp.mul_precomp_stage(mp.STAGE_POINTWISE, None, pre, None, n, n, depth, w, ws)
        torch.cuda.synchronize()
        assert torch.equal(pre, keep)
    cb = cbA.cpu().numpy().view(np.uint64)
    dig = digA.cpu().numpy().view(np.uint64)
    top = topA.cpu().numpy().astype(np.int64)
    bad = [sl for sl in range(T) if _val_reduced(dig, top, cb, sl, N) % p != want[sl]]   # (small quotient)
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]}"


@pytest.mark.parametrize("depth,w,n,has", [(8, 512, 140000, PAIR), (15, 4, 15625000, QUAD)])
def test_equals_mul_device(mp, torch_dev, depth, w, n, has):
    """mul_precomp_device(a, precomp_device(b)) == mul_device(a, b) limb for limb."""
    import torch
    _check_class(mp, n, n, depth, w, "k_pwsp<18>", (has,))
    a, b = mp.fill_random(n, 0x81 + depth), mp.fill_random(n, 0x82 + depth)
    da, db = _dev(torch, torch_dev, a), _dev(torch, torch_dev, b)
    dm = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    dp = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
    pre = mp.alloc_precomp(n, n, depth, w, torch_dev)
    mp.precomp_device(pre, db, n, n, depth, w, wsm)
    mp.mul_device(dm, da, n, db, n, depth, w, wsm)
    torch.cuda.synchronize()
    del wsm
    wsp = mp.alloc_workspace_mul_precomp(n, n, depth, w, torch_dev)
    mp.mul_precomp_device(dp, da, n, pre, n, depth, w, wsp)
    torch.cuda.synchronize()
    assert torch.equal(dp, dm)


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (11, 8, 5000)])
def test_stays_inside_workspace_and_cache(mp, oracle, torch_dev, depth, w, n):
    """Patterned guard regions behind mpfft_precomp_bytes and mpfft_mul_precomp_workspace_bytes stay
    intact, one byte less of either returns ENOMEM, and a multiply leaves the cache unchanged."""
    import torch
    lib = mp.lib()
    nbp, nbw = mp.precomp_bytes(n, n, depth, w), mp.mul_precomp_workspace_bytes(n, n, depth, w)
    assert 0 < nbw < mp.workspace_bytes(n, n, depth, w) and nbp > 0
    guard = 1 << 20
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    bufp = torch.empty(nbp + guard, dtype=torch.uint8, device=torch_dev)
    bufw = torch.empty(nbw + guard, dtype=torch.uint8, device=torch_dev)
    bufp[:nbp].fill_(0x33)
    bufw[:nbw].fill_(0x33)
    bufp[nbp:] = pat
    bufw[nbw:] = pat
    a, b = mp.fill_random(n, 0x91 + w), mp.fill_random(n, 0x92 + w)
    da, db = _dev(torch, torch_dev, a), _dev(torch, torch_dev, b)
    dr = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
    nbm = wsm.numel()
    P = lambda t: t.data_ptr()
    assert lib.mpfft_precomp_device(P(bufp), nbp - 1, P(db), n, n, depth, w, P(wsm), nbm, None) == ENOMEM
    assert lib.mpfft_precomp_device(P(bufp), nbp, P(db), n, n, depth, w, P(wsm), nbm - 1, None) == ENOMEM
    assert lib.mpfft_precomp_device(P(bufp), nbp, P(db), n, n, depth, w, P(wsm), nbm, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufp[nbp:], pat), "the precomputation wrote past mpfft_precomp_bytes"
    keep = bufp[:nbp].clone()
    assert lib.mpfft_mul_precomp_device(P(dr), P(da), n, P(bufp), nbp, n, depth, w, P(bufw), nbw - 1, None) == ENOMEM
    assert lib.mpfft_mul_precomp_device(P(dr), P(da), n, P(bufp), nbp - 1, n, depth, w, P(bufw), nbw, None) == ENOMEM
    assert lib.mpfft_mul_precomp_device(P(dr), P(da), n, P(bufp), nbp, n, depth, w, P(bufw), nbw, None) == 0
    torch.cuda.synchronize()
    assert (dr.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, b)).all()
    assert torch.equal(bufw[nbw:], pat), "the multiply wrote past mpfft_mul_precomp_workspace_bytes"
    assert torch.equal(bufp[nbp:], pat)
    assert torch.equal(bufp[:nbp], keep), "the multiply changed the cache"


@pytest.mark.parametrize("depth,w,n", [(8, 512, 40000), (11, 8, 5000)])
def test_two_streams_share_one_cache(mp, oracle, torch_dev, depth, w, n):
    """Two streams, two workspaces, one cache, different a, queued with no host sync in between."""
    import torch
    b = mp.fill_random(n, 0xa0 + w)
    a1, a2 = mp.fill_random(n, 0xa1 + w), mp.fill_random(n, 0xa2 + w)
    cb = _Cached(mp, torch_dev, b, n, depth, w)
    ws2 = mp.alloc_workspace_mul_precomp(n, n, depth, w, torch_dev)
    d1, d2 = _dev(torch, torch_dev, a1), _dev(torch, torch_dev, a2)
    r1, r2 = (torch.zeros(2 * n, dtype=torch.int64, device=torch_dev) for _ in range(2))
    s1, s2 = torch.cuda.Stream(device=torch_dev), torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    for _ in range(2):
        mp.mul_precomp_device(r1, d1, n, cb.pre, n, depth, w, cb.ws, s1)
        mp.mul_precomp_device(r2, d2, n, cb.pre, n, depth, w, ws2, s2)
    s1.synchronize()
    s2.synchronize()
    assert (r1.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a1, b)).all()
    assert (r2.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a2, b)).all()


@pytest.mark.parametrize("depth,w,n", [(7, 1024, 131064), (11, 8, 5000)])
def test_back_to_back_on_one_stream(mp, oracle, torch_dev, depth, w, n):
    """Precompute, two cached multiplies, then a plain multiply and a square on their own
    workspaces, one stream: each product's first pass has to clear the combine's look-back flags."""
    import torch
    assert mp.precomp_stage_kernels(n, n, depth, w)["combine"].startswith("k_combine1")
    a, b, c = mp.fill_random(n, 0x111), mp.fill_random(n, 0x222), mp.fill_random(n, 0x333)
    da, db, dc = (_dev(torch, torch_dev, x) for x in (a, b, c))
    r1, r2, r3, r4 = (torch.zeros(2 * n, dtype=torch.int64, device=torch_dev) for _ in range(4))
    pre = mp.alloc_precomp(n, n, depth, w, torch_dev)
    wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
    wsp = mp.alloc_workspace_mul_precomp(n, n, depth, w, torch_dev)
    wsq = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mp.precomp_device(pre, db, n, n, depth, w, wsm, st)
        mp.mul_precomp_device(r1, da, n, pre, n, depth, w, wsp, st)
        mp.mul_precomp_device(r2, dc, n, pre, n, depth, w, wsp, st)
        mp.mul_device(r3, da, n, dc, n, depth, w, wsm, st)
        mp.sqr_device(r4, dc, n, depth, w, wsq, st)
    st.synchronize()
    assert (r1.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, b)).all()
    assert (r2.cpu().numpy().view(np.uint64) == oracle.gmp_mul(c, b)).all()
    assert (r3.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, c)).all()
    assert (r4.cpu().numpy().view(np.uint64) == oracle.gmp_mul(c, c)).all()


def test_profile_covers_a_cached_multiply(mp, oracle, torch_dev):
    import torch
    depth, w, n = 8, 512, 40000
    a, b = mp.fill_random(n, 0x321), mp.fill_random(n, 0x322)
    cb = _Cached(mp, torch_dev, b, n, depth, w)
    da = _dev(torch, torch_dev, a)
    dr = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    mp.profile_begin(1)
    mp.mul_precomp_device(dr, da, n, cb.pre, n, depth, w, cb.ws)
    ms, calls = mp.profile_end()
    assert calls == 1
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert (dr.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, b)).all()


@pytest.mark.parametrize("n", [1, 7, 1000, 100000, 3000000])
def test_host_entries(mp, oracle, n):
    import torch
    a, a2, b = mp.fill_random(n, 0xabc + n), mp.fill_random(n, 0xabd + n), mp.fill_random(n, 0xabe + n)
    depth, w = mp.choose(n, n)
    with mp.Precomp(b, n, depth, w) as pre:
        assert (mp.mul_precomp(a, pre) == oracle.gmp_mul(a, b)).all(), (n, depth, w)
        assert (mp.mul_precomp(a2, pre) == oracle.gmp_mul(a2, b)).all(), (n, depth, w)   # the handle again
        with pytest.raises(mp.MpfftError) as e:   # another n1
            mp.mul_precomp(np.ones(n + 1, np.uint64), pre)
        assert e.value.code == EINVAL
        if torch.cuda.device_count() > 1:          # another device
            with torch.cuda.device(1):
                with pytest.raises(mp.MpfftError) as e:
                    mp.mul_precomp(a, pre)
            assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        mp.mul_precomp(a, pre)   # closed
    r = np.zeros(2 * n, np.uint64)
    P = lambda x: x.ctypes.data_as(mp.lib().mpfft_mul_precomp_ex.argtypes[0])
    assert mp.lib().mpfft_mul_precomp_ex(P(r), P(a), n, None) == EINVAL


def test_c_caller_precomp(mp):
    exe = os.path.join(HERE, "c_precomp", "precomp_caller")
    assert os.path.exists(exe), "tests/c_precomp/precomp_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
