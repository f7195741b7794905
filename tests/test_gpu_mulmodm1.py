"""GPU tests of the products mod M = 2^B - 1, B = 64 L (mpfft_mulmodm1_*): whole
products through every kernel family on the operands that reach the wrap, the all-ones value and
the end-around carry, the squaring entry, the device-resident chain, the split + columns, the plain
scaling and the cyclic combine alone on hand-placed slots, the cached operand, the host entries and
a plain C caller.  The reference is GMP (oracle.gmp_mul) or Python integers, folded at 2^B == 1 and
fully reduced; bit-exact is the only bar.  Every test asserts the kernel family of its shape through
mulmodm1_stage_kernels first."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # the child process of test_whole_products_pwss_at_l1024
    for d in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        sys.path.insert(0, d)

import stage_model as sm
from helpers import from_int, to_int

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def full_L(depth, w):
    """the cyclic full size: the largest bits1 <= (N - depth - 1) / 2 with 2n bits1 a multiple of 64"""
    n = 1 << depth
    b = (n * w - depth - 1) // 2
    while (2 * n * b) % 64:
        b -= 1
    return 2 * n * b // 64


def modm1(v, B):
    """v mod 2^B - 1 by folding at 2^B == 1, fully reduced"""
    mask = (1 << B) - 1
    while v >> B:
        v = (v & mask) + (v >> B)
    return 0 if v == mask else v


# (depth, w, L, pointwise starts with, forward / inverse passes start with or None): the (depth, w)
# of test_gpu_mulmod.py's table at the cyclic full size, and the same families (the split is the same)
WHOLE = [
    (4, 4, 14, "k_pointwise", None),
    (4, 4, 7, "k_pointwise", None),            # odd L, below full efficiency
    (4, 8, 30, "k_pointwise", None),
    (5, 64, 1021, "k_pw ", None),
    (6, 64, 4088, "k_pw ", ("k_lpass", "k_wpass")),
    (6, 64, 2048, "k_pw ", ("k_lpass", "k_wpass")),   # B a power of two: bits1 = N / 4
    (6, 128, 8184, "k_pwm ", None),
    (6, 192, 12280, "k_pw ", None),
    (6, 512, 32760, "k_pwm2", ("k_bpass",)),
    (5, 2048, 32765, "k_pwm2", ("k_rpass",)),
    (5, 4096, 65533, "k_pwss<18>", ("k_rpass",)),
    (6, 4096, 262136, "k_pwss<20>", ("k_rpass",)),
    (9, 256, 1048496, "k_pwss<18>", ("k_rpass",)),   # l = 2048, columns and rows in several passes each
    (8, 1024, 1048536, "k_pwss<20>", ("k_rpass",)),  # quad-fused pointwise at l = 4096, 512 slots
    (10, 128, 2096960, "k_pwss<18>", ("k_rpass",)),  # quad-fused pointwise at l = 2048, 2048 slots
    (6, 1, 56, "k_pointwise", None),
    (6, 3, 184, "k_pointwise", None),          # odd w, no sqrt2 involved
    (2, 16, 1, "k_pointwise", None),           # M = 2^64 - 1
]
PAIR, QUAD = "pair + last row level", "quad + last two row levels"
FUSED = {(6, 4096): PAIR, (9, 256): PAIR, (8, 1024): QUAD, (10, 128): QUAD}   # the later stages read C
WHOLE_IDS = ["d%d-w%d-L%d" % s[:3] for s in WHOLE]
NOT_FULL = {(4, 4, 7), (6, 64, 2048), (2, 16, 1)}


def _check_class(mp, depth, w, L, head, passes, kind=0):
    assert mp.mulmodm1_check_params(L, depth, w) == 0
    if (depth, w, L) not in NOT_FULL:
        assert L == full_L(depth, w)
    sk = mp.mulmodm1_stage_kernels(L, depth, w, kind)
    pw = sk["pointwise"]
    if head.startswith("k_pwss"):
        head = head.replace("k_pwss", ("k_pwss", "k_pwsq", "k_pwsp")[kind])
    assert pw.startswith(head), (depth, w, L, pw)
    if kind and not head.startswith("k_pws"):
        assert pw.endswith(("", "(B = A)", "(B cached)")[kind]), pw
    if passes:
        assert sk["inv_rows"].startswith(passes), sk
        assert sk["fwd_columns"].startswith(passes), sk
    assert "split" in sk["fwd_columns"], sk
    assert sk["combine"].startswith("k_combine1 + k_cwrap + k_cfix"), sk
    if (depth, w) in FUSED:
        assert FUSED[(depth, w)] in pw, sk
    else:
        assert "pair" not in pw and "quad" not in pw, sk
    return sk


def _expected(oracle, a, b, L):
    """a b mod M from the full product (GMP) folded at 2^B == 1"""
    return modm1(to_int(oracle.gmp_mul(a, b)), 64 * L)


def _operands(mp, depth, w, L, seed):
    """(name, a, b, want or None) as L-limb arrays: random, the extremes, the wraps"""
    B = 64 * L
    M = (1 << B) - 1
    b1 = B // (2 << depth)
    rng = random.Random(seed)
    ra, rb = mp.fill_random(L, seed), mp.fill_random(L, seed + 1)
    top = (2 << depth) - 1   # the last piece
    lim = lambda v: from_int(v, L)
    out = [("random", ra, rb, None),
           ("all-ones squared", lim(M), lim(M), 0),
           ("all-ones times random", lim(M), rb, 0),
           ("M-1 squared", lim(M - 1), lim(M - 1), 1),
           ("2 times 2^(B-1)", lim(2), lim(1 << (B - 1)), 1),
           ("one", lim(1), rb, None),
           ("zero", ra, lim(0), 0),
           ("top pieces", lim((rng.getrandbits(b1) | 1) << (top * b1)), lim((rng.getrandbits(b1) | 1) << (top * b1)), None)]
    if L % 2 == 0:
        out.append(("2^(B/2) - 1 times 2^(B/2) + 1", lim((1 << (B // 2)) - 1), lim((1 << (B // 2)) + 1), 0))
    return out


def _device(mp, dev, a, b, depth, w, L, ws=None, sqr=False):
    import torch
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    dr = torch.full((L,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    if ws is None:
        ws = mp.alloc_workspace_mulmodm1(L, depth, w, 1 if sqr else 0, dev)
    ws.fill_(0xFF)   # no stage may rely on zeroed memory
    if sqr:
        mp.sqrmodm1_device(dr, da, L, depth, w, ws)
    else:
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        mp.mulmodm1_device(dr, da, db, L, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _whole(mp, oracle, dev, depth, w, L, head, passes):
    sk = _check_class(mp, depth, w, L, head, passes)
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 0, dev)
    for name, a, b, fixed in _operands(mp, depth, w, L, 0x3100 + 17 * depth + w):
        got = _device(mp, dev, a, b, depth, w, L, ws)
        want = _expected(oracle, a, b, L)
        if fixed is not None:
            assert want == fixed, name
        assert to_int(got) == want, (depth, w, L, name, sk["pointwise"])
    return sk


@pytest.mark.parametrize("depth,w,L,head,passes", WHOLE, ids=WHOLE_IDS)
def test_whole_products_every_family(mp, oracle, torch_dev, depth, w, L, head, passes):
    """mulmodm1_device on every operand kind of _operands, one shape per kernel family"""
    _whole(mp, oracle, torch_dev, depth, w, L, head, passes)
    if (depth, w) == (9, 256):   # more than one pass each way
        P = mp.mulmodm1_plan_info(L, depth, w)
        assert P["NC"] >= 32 and P["NR"] >= 32, P


def test_whole_products_pwss_at_l1024(mp, torch_dev):
    """(5, 2048) through k_pwss<10>: MPFFT_POINTWISE=pwss in a fresh child process"""
    env = dict(os.environ, MPFFT_POINTWISE="pwss")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "5", "2048", "32765", "k_pwss<10>"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr


@pytest.mark.parametrize("depth,w,L,head,passes", WHOLE, ids=WHOLE_IDS)
def test_sqrmodm1(mp, oracle, torch_dev, depth, w, L, head, passes):
    """sqrmodm1_device == mulmodm1_device(a, a) == the exact value; k_pwsq on the nested plans"""
    sk = _check_class(mp, depth, w, L, head, passes, kind=1)
    if head.startswith("k_pwss"):
        assert sk["pointwise"].startswith("k_pwsq"), sk
    for name, a, b, _ in _operands(mp, depth, w, L, 0x4100 + 13 * depth + w)[:4]:
        if name == "all-ones times random":
            a = b   # the random operand
        sq = _device(mp, torch_dev, a, None, depth, w, L, sqr=True)
        mu = _device(mp, torch_dev, a, a, depth, w, L)
        assert (sq == mu).all(), (depth, w, L, name)
        assert to_int(sq) == _expected(oracle, a, a, L), (depth, w, L, name)


@pytest.mark.parametrize("depth,w,L", [(6, 64, 4088), (5, 4096, 65533)])
def test_device_chain_of_squarings(mp, torch_dev, depth, w, L):
    """x -> x^2 three times on a non-default stream, two buffers ping-ponged, no host copy between
    (the result of one call is the operand of the next); the workspace starts as 0xFF bytes and
    nothing is written past it"""
    import torch
    B = 64 * L
    x = mp.fill_random(L, 0x516)
    nb = mp.mulmodm1_workspace_bytes(L, depth, w, 1)
    guard = 1 << 16
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf.fill_(0xFF)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    ws = buf[:nb]
    b0 = torch.from_numpy(x.view(np.int64)).to(torch_dev)
    b1 = torch.full((L,), -1, dtype=torch.int64, device=torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mp.sqrmodm1_device(b1, b0, L, depth, w, ws, st)
        mp.sqrmodm1_device(b0, b1, L, depth, w, ws, st)
        mp.sqrmodm1_device(b1, b0, L, depth, w, ws, st)
    st.synchronize()
    want = to_int(x)
    for _ in range(3):
        want = modm1(want * want, B)
    assert to_int(b1.cpu().numpy().view(np.uint64)) == want
    assert torch.equal(buf[nb:], pat), "wrote past mpfft_mulmodm1_workspace_bytes"
    EINVAL, ENOMEM = 1, 4
    lib = mp.lib()
    assert lib.mpfft_sqrmodm1_device(b0.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb, None) == EINVAL
    assert lib.mpfft_sqrmodm1_device(b0.data_ptr() + 8, b0.data_ptr(), L, depth, w, ws.data_ptr(), nb, None) == EINVAL
    assert lib.mpfft_sqrmodm1_device(b1.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb - 1, None) == ENOMEM


STAGE_SHAPES = [(5, 2048, 32765), (5, 4096, 65533), (6, 4096, 262136), (6, 64, 4088), (6, 1, 56), (6, 512, 32760)]
STAGE_IDS = ["d%d-w%d-L%d" % s for s in STAGE_SHAPES]
COMBINE_SHAPES = STAGE_SHAPES + [(4, 4, 7), (6, 64, 2048), (2, 16, 1), (4, 64, 1)]
COMBINE_IDS = ["d%d-w%d-L%d" % s for s in COMBINE_SHAPES]


def _place(mp, dev, ws, L, depth, w, enc):
    """enc[j] = (limbs, pos, neg, top) into slot j of operand A's arrays"""
    import torch
    dig, top, cb = mp.mulmodm1_workspace_views(ws, L, depth, w)
    slots, l = dig.shape
    cbw = cb.shape[1]
    hd, ht, hc = np.zeros((slots, l), np.uint64), np.zeros(slots, np.int32), np.zeros((slots, cbw), np.uint64)
    for j, (limbs, pos, neg, t) in enumerate(enc):
        hd[j], ht[j], hc[j] = limbs, t, sm.pack_masks(pos, neg, cbw)
    dig.copy_(torch.from_numpy(hd.view(np.int64)).to(dev))
    top.copy_(torch.from_numpy(ht).to(dev))
    cb.copy_(torch.from_numpy(hc.view(np.int64)).to(dev))
    return dig, top, cb


def _read_slots(mp, ws, L, depth, w, which):
    """(dig, top, cb) of operand `which` as host arrays"""
    import torch
    lay = mp.mulmodm1_workspace_layout(L, depth, w)
    l = mp.mulmodm1_plan_info(L, depth, w)["l"]
    slots, cbw, k = lay["slots"], lay["cbw"], "AB"[which]
    u8 = ws.view(torch.uint8)
    torch.cuda.synchronize()
    dig = u8[lay["dig" + k]: lay["dig" + k] + slots * l * 8].cpu().numpy().view(np.uint64).reshape(slots, l)
    top = u8[lay["top" + k]: lay["top" + k] + slots * 4].cpu().numpy().view(np.int32)
    cb = u8[lay["cb" + k]: lay["cb" + k] + slots * cbw * 8].cpu().numpy().view(np.uint64).reshape(slots, cbw)
    return dig, top, cb


@pytest.mark.parametrize("depth,w,L", STAGE_SHAPES, ids=STAGE_IDS)
def test_split_and_columns_stage(mp, torch_dev, depth, w, L):
    """MPFFT_STAGE_FWD_COLUMNS (the first column pass splits) on a = all-ones (every piece full, the
    last one ending exactly at limb L) and a random b: slot (p, c) of each operand == the model's
    column transform of the unweighted pieces.  The workspace starts as 0xFF bytes."""
    import torch
    P = mp.mulmodm1_plan_info(L, depth, w)
    S = sm.Shape(P, depth, w)
    assert P["j1"] == P["j2"] == P["trunc"] == 2 * S.n and S.Tr == S.NR
    n2, b1, N, B = 2 * S.n, P["bits1"], S.N, 64 * L
    assert n2 * b1 == B
    a, b = from_int((1 << B) - 1, L), mp.fill_random(L, 0x610 + w)
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev)
    ws.fill_(0xFF)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
    dr = torch.zeros(L, dtype=torch.int64, device=torch_dev)
    mp.mulmodm1_stage(mp.STAGE_FWD_COLUMNS, da, db, dr, L, depth, w, ws)
    bad = []
    for which, v in ((0, to_int(a)), (1, to_int(b))):
        x = [(v >> (j * b1)) & ((1 << b1) - 1) for j in range(n2)]
        U = sm.fwd_columns(x, S)
        dig, top, cb = _read_slots(mp, ws, L, depth, w, which)
        for pp in range(S.NR):
            for c in range(S.NC):
                s = pp * S.NC + c
                if sm.unpack_value(dig[s], top[s], cb[s], N) % S.p != U[pp][c]:
                    bad.append((which, pp, c))
    assert not bad, f"{len(bad)} slots wrong, first {bad[:6]}"


@pytest.mark.parametrize("depth,w,L", STAGE_SHAPES, ids=STAGE_IDS)
def test_scale_stage_on_placed_slots(mp, torch_dev, depth, w, L):
    """slot j = 2^(depth+1) c_j in reduced form (carry limb in {-1, 0, 1}, +-1 carries on limbs),
    MPFFT_STAGE_SCALE: slot j must be the canonical residue of c_j -- also on the plans whose whole
    product fuses the scaling into the last inverse column pass"""
    import torch
    P = mp.mulmodm1_plan_info(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N = P["n"] * w
    p = (1 << N) + 1
    cmax = (1 << (2 * b1 + depth + 1)) - 1
    assert cmax < 1 << N
    rng = random.Random(710 + depth + w)
    fixed = [0, 1, -1, cmax, -cmax]
    cs = [fixed[j % 8] if j % 8 < 5 else rng.randint(0, cmax) for j in range(n2)]
    assert n2 >= 2 * len(sm.STYLES)
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev)
    dr = torch.zeros(L, dtype=torch.int64, device=torch_dev)
    for shift in (0, 3):   # every value class meets several encodings
        ws.fill_(0x5A)
        enc = [sm.encode_reduced(sm.modp(sm.shl(c, depth + 1, N), N), (j // 8 + j + shift) % len(sm.STYLES), l, N, rng)
               for j, c in enumerate(cs)]
        dig, top, cb = _place(mp, torch_dev, ws, L, depth, w, enc)
        mp.mulmodm1_stage(mp.STAGE_SCALE, dr, dr, dr, L, depth, w, ws)
        torch.cuda.synchronize()
        hd, ht, hc = dig.cpu().numpy().view(np.uint64), top.cpu().numpy(), cb.cpu().numpy()
        bad = []
        for j, c in enumerate(cs):
            canon = not hc[j].any() and (ht[j] == 0 or (ht[j] == 1 and not hd[j].any()))
            if not canon or to_int(hd[j]) + (int(ht[j]) << N) != c % p:
                bad.append((j, c if abs(c) < 2 else "big", canon))
        assert not bad, f"{len(bad)} of {n2} slots wrong, first {bad[:6]}"


def _combine_patterns(n2, b1, depth, N, B, rng, extreme):
    """(name, coefficients, want or None); 0 <= c_j < 2^N"""
    o = (1 << b1) - 1
    cmax = (1 << (2 * b1 + depth + 1)) - 1
    M = (1 << B) - 1
    z = [0] * n2
    q = b1 + depth
    out = [("all o: the sum is all-ones", [o] * n2, 0),
           ("all o, plus 2^bits1 on the last: the chain carries through every limb", [o] * (n2 - 1) + [o + (1 << b1)], 1),
           ("only c_last = 2^bits1", z[:-1] + [1 << b1], 1),
           ("o - 1, then all o: M - 1 stays", [o - 1] + [o] * (n2 - 1), M - 1),
           ("all o, plus 2^(bits1+q) on the last: the end-around carry passes all-ones limbs",
            [o] * (n2 - 1) + [o + (1 << (b1 + q))], (1 << q) % M),
           ("all 2^(2 bits1) - 1: a multiple of M", [(1 << (2 * b1)) - 1] * n2, 0),
           ("all cmax", [cmax] * n2, None),
           ("last cmax", z[:-1] + [cmax], None),
           ("random", [rng.randint(0, cmax) for _ in range(n2)], None),
           ("zero", z, 0)]
    if extreme:
        out.append(("all 2^N - 1", [(1 << N) - 1] * n2, 0))
    return out


@pytest.mark.parametrize("depth,w,L", COMBINE_SHAPES, ids=COMBINE_IDS)
def test_combine_stage_on_placed_coefficients(mp, torch_dev, depth, w, L):
    """canonical coefficients 0 <= c_j < 2^N placed, MPFFT_STAGE_COMBINE: r == sum c_j 2^(j bits1)
    mod M, fully reduced (the workspace's flags and scratch start as 0x5A bytes).  At (4, 64, 1)
    N = 1024 against B = 64: 17 pieces of the scratch sum."""
    import torch
    P = mp.mulmodm1_plan_info(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N, B = P["n"] * w, 64 * L
    assert mp.mulmodm1_stage_kernels(L, depth, w)["combine"].startswith("k_combine1 + k_cwrap + k_cfix")
    if (depth, w, L) == (4, 64, 1):
        assert -(-((n2 - 1) * b1 + N) // 64) == 17
    rng = random.Random(910 + depth + w)
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev)
    dr = torch.zeros(L, dtype=torch.int64, device=torch_dev)
    for name, cs, fixed in _combine_patterns(n2, b1, depth, N, B, rng, (depth, w, L) in ((4, 64, 1), (2, 16, 1))):
        assert all(0 <= c < 1 << N for c in cs), name
        ws.fill_(0x5A)
        dr.fill_(0x5A5A)
        _place(mp, torch_dev, ws, L, depth, w, [(from_int(c, l), (), (), 0) for c in cs])
        mp.mulmodm1_stage(mp.STAGE_COMBINE, dr, dr, dr, L, depth, w, ws)
        torch.cuda.synchronize()
        want = modm1(sum(c << (j * b1) for j, c in enumerate(cs)), B)
        if fixed is not None:
            assert want == fixed, (depth, w, L, name)
        got = dr.cpu().numpy().view(np.uint64)
        assert to_int(got) == want, (depth, w, L, name)


def test_stage_entry_rejects_the_multiply_only_stages(mp, torch_dev):
    import torch
    depth, w, L = 6, 64, 4088
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev)
    d = torch.zeros(L, dtype=torch.int64, device=torch_dev)
    for stage in (mp.STAGE_FOLD_COMBINE, mp.STAGE_SCALE | mp.STAGE_DRIVEN, mp.STAGE_INV_ROWS | mp.STAGE_DRIVEN):
        with pytest.raises(mp.MpfftError) as e:
            mp.mulmodm1_stage(stage, d, d, d, L, depth, w, ws)
        assert e.value.code == 1


PRE_SHAPES = [(6, 512, 32760, "k_pwm2"), (5, 4096, 65533, "k_pwss<18>"), (6, 4096, 262136, "k_pwss<20>"),
              (8, 1024, 1048536, "k_pwss<20>")]   # one per pointwise class: not nested, FUSE 0, 1, 2


@pytest.mark.parametrize("depth,w,L,head", PRE_SHAPES, ids=["d%d-w%d-L%d" % s[:3] for s in PRE_SHAPES])
def test_cached_operand(mp, oracle, torch_dev, depth, w, L, head):
    """one cache of b reused across three different a: limb-equal to mulmodm1_device and exact; a
    cache or workspace one byte short is refused"""
    import torch
    _check_class(mp, depth, w, L, head, None, kind=2)
    b = mp.fill_random(L, 0x7b0 + depth)
    db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
    wsm = mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev)
    wsp = mp.alloc_workspace_mulmodm1(L, depth, w, 2, torch_dev)
    assert wsp.numel() == mp.mulmodm1_workspace_bytes(L, depth, w, 1) < wsm.numel()
    pre = mp.alloc_precomp_mulmodm1(L, depth, w, torch_dev)
    wsm.fill_(0xFF)
    pre.fill_(0x5A)
    mp.mulmodm1_precomp_device(pre, db, L, depth, w, wsm)
    torch.cuda.synchronize()
    snap = pre.clone()
    M = (1 << (64 * L)) - 1
    for k, a in enumerate((mp.fill_random(L, 0x7a0 + k) for k in range(2))):
        da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
        dr = torch.full((L,), 0x5A5A, dtype=torch.int64, device=torch_dev)
        dm = torch.full((L,), 0x5A5A, dtype=torch.int64, device=torch_dev)
        wsp.fill_(0xFF if k else 0x5A)
        wsm.fill_(0xFF)
        mp.mulmodm1_mul_precomp_device(dr, da, pre, L, depth, w, wsp)
        mp.mulmodm1_device(dm, da, db, L, depth, w, wsm)
        torch.cuda.synchronize()
        assert torch.equal(dr, dm), (depth, w, L, k)
        assert to_int(dr.cpu().numpy().view(np.uint64)) == _expected(oracle, a, b, L)
    a = from_int(M, L)   # the third a: all-ones, 0 mod M
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.full((L,), 0x5A5A, dtype=torch.int64, device=torch_dev)
    mp.mulmodm1_mul_precomp_device(dr, da, pre, L, depth, w, wsp)
    torch.cuda.synchronize()
    assert not dr.any()
    assert torch.equal(pre, snap), "a multiply wrote to the cache"
    ENOMEM = 4
    lib = mp.lib()
    pb, wb, mb = pre.numel(), wsp.numel(), wsm.numel()
    assert lib.mpfft_mulmodm1_mul_precomp_device(dr.data_ptr(), da.data_ptr(), pre.data_ptr(), pb - 1, L, depth, w,
                                                 wsp.data_ptr(), wb, None) == ENOMEM
    assert lib.mpfft_mulmodm1_mul_precomp_device(dr.data_ptr(), da.data_ptr(), pre.data_ptr(), pb, L, depth, w,
                                                 wsp.data_ptr(), wb - 1, None) == ENOMEM
    assert lib.mpfft_mulmodm1_precomp_device(pre.data_ptr(), pb - 1, db.data_ptr(), L, depth, w, wsm.data_ptr(), mb, None) == ENOMEM
    assert lib.mpfft_mulmodm1_precomp_device(pre.data_ptr(), pb, db.data_ptr(), L, depth, w, wsm.data_ptr(), mb - 1, None) == ENOMEM


def test_two_streams_share_one_cache(mp, oracle, torch_dev):
    """two streams, two workspaces, one cache, different a, queued with no host sync in between"""
    import torch
    depth, w, L = 6, 4096, 262136
    b = mp.fill_random(L, 0x7c0)
    db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
    pre = mp.alloc_precomp_mulmodm1(L, depth, w, torch_dev)
    mp.mulmodm1_precomp_device(pre, db, L, depth, w, mp.alloc_workspace_mulmodm1(L, depth, w, 0, torch_dev))
    torch.cuda.synchronize()
    As = [mp.fill_random(L, 0x7d0 + k) for k in range(2)]
    das = [torch.from_numpy(a.view(np.int64)).to(torch_dev) for a in As]
    drs = [torch.zeros(L, dtype=torch.int64, device=torch_dev) for _ in As]
    wss = [mp.alloc_workspace_mulmodm1(L, depth, w, 2, torch_dev) for _ in As]
    sts = [torch.cuda.Stream(device=torch_dev) for _ in As]
    torch.cuda.synchronize()
    for _ in range(2):
        for k in range(2):
            with torch.cuda.stream(sts[k]):
                mp.mulmodm1_mul_precomp_device(drs[k], das[k], pre, L, depth, w, wss[k], sts[k])
    for st in sts:
        st.synchronize()
    for k in range(2):
        assert to_int(drs[k].cpu().numpy().view(np.uint64)) == _expected(oracle, As[k], b, L), k


@pytest.mark.parametrize("L", [1, 14, 1000, 100000])
def test_host_entries(mp, oracle, L):
    """mulmodm1 / sqrmodm1 on host arrays at mulmodm1_choose's pair; every operand value is valid"""
    depth, w = mp.mulmodm1_choose(L)
    assert mp.mulmodm1_check_params(L, depth, w) == 0
    a, b = mp.fill_random(L, 0xa1 + L), mp.fill_random(L, 0xb1 + L)
    assert to_int(mp.mulmodm1(a, b, depth, w)) == _expected(oracle, a, b, L), (L, depth, w)
    assert to_int(mp.sqrmodm1(a, depth, w)) == _expected(oracle, a, a, L), (L, depth, w)
    ones = from_int((1 << (64 * L)) - 1, L)
    assert not mp.mulmodm1(ones, b, depth, w).any()
    assert not mp.sqrmodm1(ones, depth, w).any()
    assert to_int(mp.sqrmodm1(from_int((1 << (64 * L)) - 2, L), depth, w)) == 1


def test_next_size_product(mp, oracle):
    L, depth, w = mp.mulmodm1_next_size(5000)
    assert L >= 5000 and mp.mulmodm1_check_params(L, depth, w) == 0
    a, b = mp.fill_random(L, 1), mp.fill_random(L, 2)
    assert to_int(mp.mulmodm1(a, b, depth, w)) == _expected(oracle, a, b, L)


def test_profile_covers_mulmodm1(mp, torch_dev):
    import torch
    depth, w, L = 6, 512, 32760
    a = mp.fill_random(L, 0x322)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.zeros(L, dtype=torch.int64, device=torch_dev)
    ws = mp.alloc_workspace_mulmodm1(L, depth, w, 1, torch_dev)
    mp.profile_begin(1)
    mp.sqrmodm1_device(dr, da, L, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == 1
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert to_int(dr.cpu().numpy().view(np.uint64)) == modm1(to_int(a) ** 2, 64 * L)


def test_c_caller_mulmodm1(mp):
    exe = os.path.join(HERE, "c_mulmodm1", "mulmodm1_caller")
    assert os.path.exists(exe), "tests/c_mulmodm1/mulmodm1_caller not built (run __graft_entry__.build())"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr


if __name__ == "__main__":
    import torch

    import mpfft_loader
    import oracle as O
    d_, w_, L_, head_ = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    if not torch.cuda.is_available():
        print("no GPU")
        sys.exit(2)
    _whole(mpfft_loader.load(), O, torch.device("cuda:0"), d_, w_, L_, head_, ("k_rpass",))
    print("OK")
