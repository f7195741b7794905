"""GPU tests of the squaring entries (mpfft_sqr_*): whole squares through every pointwise class
(k_pwsq<10/18/20> at FUSE 0, 1, 2, and the multiply kernels run with B = A), the pointwise stage
alone on hand-placed residues, equality with the multiply, the smaller workspace, the host
entries, profiling and a plain C caller.  The reference is GMP (oracle.gmp_mul(a, a)) or exact
integer arithmetic; bit-exact is the only bar.  Every test asserts the kernel class of its shape
through sqr_stage_kernels first, so a planner change cannot silently move it."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import max_limbs, to_int

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _pointwise_env:
    """MPFFT_POINTWISE set (or unset for None) inside the block, restored afterwards"""

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


def _check_class(mp, n, depth, w, pw_head, pw_has=(), scale=None, combine=None, whole=True):
    sk = mp.sqr_stage_kernels(n, depth, w)
    pw = sk["pointwise"]
    assert pw.startswith(pw_head), (depth, w, n, pw)
    for s in pw_has:
        assert s in pw, (depth, w, n, pw)
    if whole and pw_head.startswith("k_pwsq") and not pw_has:
        assert "pair" not in pw and "quad" not in pw, pw   # FUSE 0 (the stage entry never fuses row levels)
    if not pw_head.startswith("k_pwsq"):
        assert pw.endswith("(B = A)"), pw
    if scale:
        assert sk["scale"].startswith(scale), sk["scale"]
    if combine:
        assert sk["combine"].startswith(combine), sk["combine"]
    return sk


def _sqr_device(mp, dev, a, depth, w, ws=None):
    import torch
    n = len(a)
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    dr = torch.zeros(2 * n, dtype=torch.int64, device=dev)
    if ws is None:
        ws = mp.alloc_workspace_sqr(n, depth, w, dev)
    mp.sqr_device(dr, da, n, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _case_b(mp, n, depth, w):
    P = mp.plan_info(n, n, depth, w)
    return P["trunc"] > P["n"]


PAIR, QUAD = "pair + last row level", "quad + last two row levels"
FOLD = "k_cmeta + k_combine_red"
# (depth, w, n, MPFFT_POINTWISE, pointwise starts with, pointwise contains, scale, combine, case b)
WHOLE = [
    (7, 1024, 131064, None, "k_pwsq<18>", (), "k_rscale", "k_combine1", None),
    (5, 4096, 20000, None, "k_pwsq<18>", (), "(folded", FOLD, True),
    (6, 2048, 40000, None, "k_pwsq<18>", (), "(folded", FOLD, True),
    (8, 512, 40000, None, "k_pwsq<18>", (PAIR,), None, None, None),
    (8, 512, 140000, None, "k_pwsq<18>", (PAIR,), None, None, True),
    (14, 8, 500000, None, "k_pwsq<18>", (QUAD,), None, None, None),
    (12, 64, 500000, None, "k_pwsq<20>", (), None, None, None),
    (6, 4096, 131064, None, "k_pwsq<20>", (PAIR,), "k_rscale", "k_combine1", None),
    (7, 2048, 150000, None, "k_pwsq<20>", (PAIR,), "(folded", FOLD, True),
    (16, 4, 500000, None, "k_pwsq<20>", (QUAD,), None, None, None),
    (6, 1024, 32760, "pwss", "k_pwsq<10>", (), None, None, None),
    (9, 2, 120, None, "k_pointwise", (), None, None, None),
    (11, 8, 5000, None, "k_pwm2", (), None, None, None),
    (9, 64, 30000, None, "k_pwm2", (), None, None, None),
    (9, 16, None, None, "k_pwm ", (), None, None, None),     # l = 128, n = max_limbs
    (8, 8, None, None, "k_pw ", (), None, None, None),       # l = 32, n = max_limbs
]


@pytest.mark.parametrize("depth,w,n,kind,head,has,scale,combine,caseb", WHOLE)
def test_whole_squares_every_pointwise_class(mp, oracle, torch_dev, depth, w, n, kind, head, has, scale, combine, caseb):
    if n is None:
        n = max_limbs(depth, w)
    with _pointwise_env(kind):
        sk = _check_class(mp, n, depth, w, head, has, scale, combine)
        if caseb:
            assert _case_b(mp, n, depth, w)
        if (depth, w, n) == (8, 512, 140000):
            assert "FILL + half-add" in sk["inv_columns"], sk["inv_columns"]
        if (depth, w) == (11, 8):
            assert sk["fwd_columns"].startswith("k_lpass") or sk["fwd_columns"].startswith("k_wpass"), sk
        if (depth, w) == (9, 64):
            assert sk["fwd_columns"].startswith("k_bpass"), sk
        ws = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
        for a in (mp.fill_random(n, 0x5000 + 31 * depth + w), np.full(n, 2**64 - 1, dtype=np.uint64)):
            got = _sqr_device(mp, torch_dev, a, depth, w, ws)
            assert (got == oracle.gmp_mul(a, a)).all(), (depth, w, n, sk["pointwise"])


def _pattern(kind, l, N, rng):
    """canonical residues (limbs, top) that stress the pointwise kernels"""
    if kind == 1:
        return 0, 1                                          # 2^N == -1
    v = {0: rng.getrandbits(N), 2: (1 << N) - 1, 3: 0, 4: 1,
         5: int.from_bytes(b"\x80" * (8 * l), "little"), 6: int.from_bytes(b"\x7f" * (8 * l), "little"),
         7: (1 << N) - 1 - rng.getrandbits(64)}[kind]
    return v, 0


def _modp(x, N):
    """x mod 2^N + 1 for 0 <= x < 2^(3N) by folding (2^N == -1): a full-length division costs
    seconds over a test's slots at l = 4096"""
    m = (1 << N) - 1
    return ((x & m) - ((x >> N) & m) + (x >> (2 * N))) % (m + 2)


def _val_reduced(dig, top, cb, s, N):
    """value of a reduced-form slot: limbs + carries (limb m's carry lands at 2^(64(m+1))) + top 2^N"""
    l = dig.shape[1]

    def carries(words):   # bit k of mask word W set: limb 64 W + k carries into limb 64 W + k + 1
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
        assert not bits[l:].any()
        z = np.zeros(l + 1, np.uint64)
        z[1:] = bits[:l]
        return to_int(z)
    return to_int(dig[s]) + int(top[s]) * (1 << N) + carries(cb[s][0::2]) - carries(cb[s][1::2])


@pytest.mark.parametrize("depth,w,kind,head", [(5, 4096, None, "k_pwsq<18>"), (6, 4096, None, "k_pwsq<20>"),
                                               (6, 1024, "pwss", "k_pwsq<10>"), (9, 16, None, "k_pwm "),
                                               (8, 64, None, "k_pwm2"), (11, 1, None, "k_pw ")])
def test_sqr_pointwise_stage_on_placed_values(mp, torch_dev, depth, w, kind, head):
    """The pointwise stage alone (sqr_stage) on hand-placed canonical residues in the square
    workspace's A slots: every live slot against v^2 mod 2^N + 1."""
    import torch
    n = max_limbs(depth, w)
    P = mp.plan_info(n, n, depth, w)
    l, T, N = P["l"], P["trunc"], P["n"] * w
    p = (1 << N) + 1
    rng = random.Random(depth * 1000 + w)
    with _pointwise_env(kind):
        _check_class(mp, n, depth, w, head, whole=False)
        ws = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
        ws.fill_(0)
        digA, topA = mp.sqr_workspace_views(ws, n, depth, w)
        want = []
        hd, ht = np.zeros((T, l), np.uint64), np.zeros(T, np.int32)
        for sl in range(T):
            v, t = _pattern(sl % 8, l, N, rng)
            hd[sl] = np.frombuffer(v.to_bytes(8 * l, "little"), dtype=np.uint64)
            ht[sl] = t
            want.append(_modp((v + t * (1 << N)) ** 2, N))
        assert T >= 8   # every pattern kind is placed
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
    bad = [sl for sl in range(T) if _val_reduced(dig, top, cb, sl, N) % p != want[sl]]   # (small quotient)
    assert not bad, f"{len(bad)} of {T} slots wrong, first {bad[:8]}"


@pytest.mark.parametrize("depth,w,n,gmp", [(8, 512, 140000, True), (15, 4, 15625000, False)])
def test_sqr_equals_mul_of_a_by_a(mp, oracle, torch_dev, depth, w, n, gmp):
    """sqr_device(a) == mul_device(a, a) limb for limb (the second shape -- the only l = 2048 quad
    shape with a full-length inverse -- relies on the already-tested multiply alone)."""
    import torch
    _check_class(mp, n, depth, w, "k_pwsq<18>", (PAIR,) if depth == 8 else (QUAD,))
    a = mp.fill_random(n, 0x77 + depth)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dm = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    ws = mp.alloc_workspace(n, n, depth, w, torch_dev)
    mp.mul_device(dm, da, n, da, n, depth, w, ws)
    torch.cuda.synchronize()
    del ws
    ds = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    wsq = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
    mp.sqr_device(ds, da, n, depth, w, wsq)
    torch.cuda.synchronize()
    assert torch.equal(ds, dm)
    if gmp:
        assert (ds.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, a)).all()


@pytest.mark.parametrize("depth,w,n", [(8, 512, 140000), (11, 8, 5000)])
def test_sqr_stays_inside_its_smaller_workspace(mp, oracle, torch_dev, depth, w, n):
    import torch
    nb = mp.sqr_workspace_bytes(n, depth, w)
    assert 0 < nb < mp.workspace_bytes(n, n, depth, w)
    guard = 1 << 20
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf[:nb].fill_(0x33)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    a = mp.fill_random(n, 0x99 + w)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    rc = mp.lib().mpfft_sqr_device(dr.data_ptr(), da.data_ptr(), n, depth, w, buf.data_ptr(), nb, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert (dr.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, a)).all()
    assert torch.equal(buf[nb:], pat), "the square wrote past mpfft_sqr_workspace_bytes"
    ENOMEM = 4
    assert mp.lib().mpfft_sqr_device(dr.data_ptr(), da.data_ptr(), n, depth, w, buf.data_ptr(), nb - 1, None) == ENOMEM


@pytest.mark.parametrize("n", [1, 7, 1000, 100000, 3000000])
def test_host_entries(mp, oracle, n):
    a = mp.fill_random(n, 0xabc + n)
    want = oracle.gmp_mul(a, a)
    depth, w = mp.choose(n, n)
    assert (mp.sqr(a, depth, w) == want).all(), (n, depth, w)
    assert (mp.sqr_auto(a) == want).all(), n


@pytest.mark.parametrize("depth,w,n", [(7, 1024, 131064), (11, 8, 5000)])
def test_back_to_back_squares_then_a_multiply(mp, oracle, torch_dev, depth, w, n):
    """Two squares queued on one stream with one workspace, then a multiply on the multiply's
    workspace: each call's first pass has to clear the combine's look-back flags again."""
    import torch
    assert mp.sqr_stage_kernels(n, depth, w)["combine"].startswith("k_combine1")
    a, b = mp.fill_random(n, 0x111), mp.fill_random(n, 0x222)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
    r1, r2, r3 = (torch.zeros(2 * n, dtype=torch.int64, device=torch_dev) for _ in range(3))
    wsq = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
    wsm = mp.alloc_workspace(n, n, depth, w, torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mp.sqr_device(r1, da, n, depth, w, wsq, st)
        mp.sqr_device(r2, db, n, depth, w, wsq, st)
        mp.mul_device(r3, da, n, db, n, depth, w, wsm, st)
    st.synchronize()
    assert (r1.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, a)).all()
    assert (r2.cpu().numpy().view(np.uint64) == oracle.gmp_mul(b, b)).all()
    assert (r3.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, b)).all()


def test_profile_covers_squares(mp, oracle, torch_dev):
    import torch
    depth, w, n = 8, 512, 40000
    a = mp.fill_random(n, 0x321)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.zeros(2 * n, dtype=torch.int64, device=torch_dev)
    ws = mp.alloc_workspace_sqr(n, depth, w, torch_dev)
    mp.profile_begin(1)
    mp.sqr_device(dr, da, n, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == 1
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert (dr.cpu().numpy().view(np.uint64) == oracle.gmp_mul(a, a)).all()


def test_c_caller_sqr(mp):
    exe = os.path.join(HERE, "c_sqr", "sqr_caller")
    assert os.path.exists(exe), "tests/c_sqr/sqr_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
