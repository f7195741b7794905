"""GPU tests of the products mod M = 2^B + 1, B = 64 L (mpfft_mulmod_*): whole
products through every kernel family on the operands that reach the wraps and both coefficient
signs, the squaring entry, the device-resident chain, the un-weight and the negacyclic combine
alone on hand-placed slots, the host entries and a plain C caller.  The reference is GMP
(oracle.gmp_mul) or Python integers, folded at 2^B == -1; bit-exact is the only bar.  Every test
asserts the kernel family of its shape through mulmod_stage_kernels first."""
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
    """the largest L of (depth, w): bits1 <= (N - depth - 2) / 2 with 2n bits1 a multiple of 64"""
    n = 1 << depth
    b = (n * w - depth - 2) // 2
    while (2 * n * b) % 64:
        b -= 1
    return 2 * n * b // 64


# (depth, w, L, pointwise starts with, forward passes start with or None)
WHOLE = [
    (4, 4, 14, "k_pointwise", None),
    (4, 4, 7, "k_pointwise", None),            # odd L, below full efficiency: 2^64 + 1 divides M
    (4, 8, 30, "k_pointwise", None),
    (5, 64, 1020, "k_pw ", None),
    (6, 64, 4088, "k_pw ", ("k_lpass", "k_wpass")),
    (6, 64, 2048, "k_pw ", ("k_lpass", "k_wpass")),   # L below full efficiency: bits1 = N / 4
    (6, 128, 8184, "k_pwm ", None),
    (6, 192, 12280, "k_pw ", None),
    (6, 512, 32760, "k_pwm2", ("k_bpass",)),
    (5, 2048, 32764, "k_pwm2", ("k_rpass",)),
    (5, 4096, 65532, "k_pwss<18>", ("k_rpass",)),
    (6, 4096, 262136, "k_pwss<20>", ("k_rpass",)),
    (9, 256, 1048480, "k_pwss<18>", ("k_rpass",)),   # l = 2048, columns and rows in several passes each
    (8, 1024, 1048536, "k_pwss<20>", ("k_rpass",)),  # quad-fused pointwise at l = 4096, 512 slots
    (10, 128, 2096960, "k_pwss<18>", ("k_rpass",)),  # quad-fused pointwise at l = 2048, 2048 slots
    (6, 1, 56, "k_pointwise", None),           # odd w: theta = sqrt2
]
PAIR, QUAD = "pair + last row level", "quad + last two row levels"
FUSED = {(6, 4096): PAIR, (9, 256): PAIR, (8, 1024): QUAD, (10, 128): QUAD}   # the later stages read C
WHOLE_IDS = ["d%d-w%d-L%d" % s[:3] for s in WHOLE]
FULL = {(4, 4, 14), (4, 8, 30), (5, 64, 1020), (6, 64, 4088), (6, 128, 8184), (6, 192, 12280), (6, 512, 32760),
        (5, 2048, 32764), (5, 4096, 65532), (6, 4096, 262136), (9, 256, 1048480), (6, 1, 56), (8, 1024, 1048536),
        (10, 128, 2096960)}


def _check_class(mp, depth, w, L, head, passes, sqr=False):
    assert mp.mulmod_check_params(L, depth, w) == 0
    if (depth, w, L) in FULL:
        assert L == full_L(depth, w)
    sk = mp.mulmod_stage_kernels(L, depth, w, sqr)
    pw = sk["pointwise"]
    if sqr and head.startswith("k_pwss"):
        head = head.replace("k_pwss", "k_pwsq")
    assert pw.startswith(head), (depth, w, L, pw)
    if sqr and not head.startswith("k_pwsq"):
        assert pw.endswith("(B = A)"), pw
    if passes:
        assert sk["inv_rows"].startswith(passes), sk
    assert sk["fwd_columns"].startswith("k_nweight<"), sk
    assert "k_nwrap" in sk["combine"], sk
    if passes == ("k_rpass",) and w % 2 == 0:
        assert sk["scale"].startswith("k_rscale"), sk
    else:
        assert sk["scale"].startswith("k_nunweight<"), sk
    return sk


def _limbs(v, L):
    return from_int(v, L + 1)


def _expected(oracle, a, b, L):
    """a b mod M from the full product (GMP) folded at 2^B == -1"""
    return sm.modp(to_int(oracle.gmp_mul(a, b)), 64 * L)


def _operands(mp, depth, w, L, seed):
    """(name, a, b) as L + 1-limb arrays: random, the reduced extremes, the wraps, both signs"""
    B = 64 * L
    M = (1 << B) + 1
    b1 = B // (2 << depth)
    rng = random.Random(seed)
    ra, rb = mp.fill_random(L + 1, seed), mp.fill_random(L + 1, seed + 1)
    ra[L] = rb[L] = 0
    top = (2 << depth) - 1   # the last piece
    out = [("random", ra, rb),
           ("2^B squared", _limbs(1 << B, L), _limbs(1 << B, L)),
           ("2^B times random", _limbs(1 << B, L), rb),
           ("2^B-1 squared", _limbs((1 << B) - 1, L), _limbs((1 << B) - 1, L)),
           ("2 times 2^(B-1)", _limbs(2, L), _limbs(1 << (B - 1), L)),
           ("one", _limbs(1, L), rb),
           ("zero", ra, _limbs(0, L)),
           ("top pieces", _limbs(rng.getrandbits(b1) << (top * b1), L), _limbs((rng.getrandbits(b1) | 1) << (top * b1), L))]
    if L % 2:
        f = (1 << 64) + 1
        assert M % f == 0
        out.append(("a factor times its cofactor", _limbs(f, L), _limbs(M // f, L)))
    return out


def _mulmod_device(mp, dev, a, b, depth, w, L, ws=None, sqr=False):
    import torch
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    dr = torch.full((L + 1,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    if ws is None:
        ws = mp.alloc_workspace_mulmod(L, depth, w, sqr, dev)
    ws.fill_(0xFF)   # no stage may rely on zeroed memory
    if sqr:
        mp.sqrmod_device(dr, da, L, depth, w, ws)
    else:
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        mp.mulmod_device(dr, da, db, L, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _whole(mp, oracle, dev, depth, w, L, head, passes):
    sk = _check_class(mp, depth, w, L, head, passes)
    B = 64 * L
    ws = mp.alloc_workspace_mulmod(L, depth, w, False, dev)
    for name, a, b in _operands(mp, depth, w, L, 0x3000 + 17 * depth + w):
        got = _mulmod_device(mp, dev, a, b, depth, w, L, ws)
        want = _expected(oracle, a, b, L)
        assert to_int(got) == want, (depth, w, L, name, sk["pointwise"])
        assert got[L] == (1 if want == 1 << B else 0)
        if name == "2^B times random":
            assert want == (1 << B) + 1 - to_int(b)
        elif name == "2 times 2^(B-1)":
            assert want == 1 << B and got[L] == 1 and not got[:L].any()
        elif name == "a factor times its cofactor":
            assert want == 0
    return sk


@pytest.mark.parametrize("depth,w,L,head,passes", WHOLE, ids=WHOLE_IDS)
def test_whole_products_every_family(mp, oracle, torch_dev, depth, w, L, head, passes):
    """mulmod_device on every operand kind of _operands, one shape per kernel family"""
    sk = _whole(mp, oracle, torch_dev, depth, w, L, head, passes)
    if (depth, w) == (9, 256):   # more than one pass each way
        P = mp.mulmod_plan_info(L, depth, w)
        assert P["NC"] >= 32 and P["NR"] >= 32, P
    if (depth, w) in FUSED:
        assert FUSED[(depth, w)] in sk["pointwise"], sk
    else:
        assert "pair" not in sk["pointwise"] and "quad" not in sk["pointwise"], sk


def test_whole_products_pwss_at_l1024(mp, torch_dev):
    """(5, 2048) through k_pwss<10>: MPFFT_POINTWISE=pwss in a fresh child process"""
    env = dict(os.environ, MPFFT_POINTWISE="pwss")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "5", "2048", "32764", "k_pwss<10>"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr


@pytest.mark.parametrize("depth,w,L,head,passes", WHOLE, ids=WHOLE_IDS)
def test_sqrmod(mp, oracle, torch_dev, depth, w, L, head, passes):
    """sqrmod_device == mulmod_device(a, a) == the exact value; k_pwsq on the nested plans"""
    sk = _check_class(mp, depth, w, L, head, passes, sqr=True)
    if head.startswith("k_pwss"):
        assert sk["pointwise"].startswith("k_pwsq"), sk
    B = 64 * L
    for name, a, b in _operands(mp, depth, w, L, 0x4000 + 13 * depth + w)[:4]:
        if name == "2^B times random":
            a = b   # the random operand
        sq = _mulmod_device(mp, torch_dev, a, None, depth, w, L, sqr=True)
        mu = _mulmod_device(mp, torch_dev, a, a, depth, w, L)
        assert (sq == mu).all(), (depth, w, L, name)
        assert to_int(sq) == _expected(oracle, a, a, L), (depth, w, L, name)


@pytest.mark.parametrize("depth,w,L", [(6, 64, 4088), (5, 4096, 65532)])
def test_device_chain_of_squarings(mp, torch_dev, depth, w, L):
    """x -> x^2 three times on a non-default stream, two buffers ping-ponged, no host copy between
    (the result of one call is the operand of the next); the workspace starts as 0xFF bytes and
    nothing is written past it"""
    import torch
    B = 64 * L
    x = mp.fill_random(L + 1, 0x515)
    x[L] = 0
    nb = mp.mulmod_workspace_bytes(L, depth, w, True)
    guard = 1 << 16
    buf = torch.empty(nb + guard, dtype=torch.uint8, device=torch_dev)
    buf.fill_(0xFF)
    pat = torch.arange(guard, device=torch_dev, dtype=torch.int32).mul_(37).add_(11).to(torch.uint8)
    buf[nb:] = pat
    ws = buf[:nb]
    b0 = torch.from_numpy(x.view(np.int64)).to(torch_dev)
    b1 = torch.full((L + 1,), -1, dtype=torch.int64, device=torch_dev)
    st = torch.cuda.Stream(device=torch_dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        mp.sqrmod_device(b1, b0, L, depth, w, ws, st)
        mp.sqrmod_device(b0, b1, L, depth, w, ws, st)
        mp.sqrmod_device(b1, b0, L, depth, w, ws, st)
    st.synchronize()
    want = to_int(x)
    for _ in range(3):
        want = sm.modp(want * want, B)
    assert to_int(b1.cpu().numpy().view(np.uint64)) == want
    assert torch.equal(buf[nb:], pat), "wrote past mpfft_mulmod_workspace_bytes"
    EINVAL, ENOMEM = 1, 4
    lib = mp.lib()
    assert lib.mpfft_sqrmod_device(b0.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb, None) == EINVAL
    assert lib.mpfft_sqrmod_device(b1.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb - 1, None) == ENOMEM


STAGE_SHAPES = [(5, 2048, 32764), (5, 4096, 65532), (6, 4096, 262136), (6, 64, 4088), (6, 1, 56)]
STAGE_IDS = ["d%d-w%d-L%d" % s for s in STAGE_SHAPES]


def _place(mp, dev, ws, L, depth, w, enc):
    """enc[j] = (limbs, pos, neg, top) into slot j of operand A's arrays"""
    import torch
    dig, top, cb = mp.mulmod_workspace_views(ws, L, depth, w)
    slots, l = dig.shape
    cbw = cb.shape[1]
    hd, ht, hc = np.zeros((slots, l), np.uint64), np.zeros(slots, np.int32), np.zeros((slots, cbw), np.uint64)
    for j, (limbs, pos, neg, t) in enumerate(enc):
        hd[j], ht[j], hc[j] = limbs, t, sm.pack_masks(pos, neg, cbw)
    dig.copy_(torch.from_numpy(hd.view(np.int64)).to(dev))
    top.copy_(torch.from_numpy(ht).to(dev))
    cb.copy_(torch.from_numpy(hc.view(np.int64)).to(dev))
    return dig, top, cb


def _theta(c, j, w, N, e=0):
    """theta^j 2^e c mod p, theta = sqrt2^w"""
    if (j * w) % 2 == 0:
        return sm.modp(sm.shl(c, j * w // 2 + e, N), N)
    sqrt2 = (1 << (3 * N // 4)) - (1 << (N // 4))
    return sm.modp(sm.shl(c * sqrt2, (j * w - 1) // 2 + e, N), N)


def _read_slots(mp, ws, L, depth, w, which):
    """(dig, top, cb) of operand `which` as host arrays"""
    import torch
    lay = mp.mulmod_workspace_layout(L, depth, w)
    l = mp.mulmod_plan_info(L, depth, w)["l"]
    slots, cbw, k = lay["slots"], lay["cbw"], "AB"[which]
    u8 = ws.view(torch.uint8)
    torch.cuda.synchronize()
    dig = u8[lay["dig" + k]: lay["dig" + k] + slots * l * 8].cpu().numpy().view(np.uint64).reshape(slots, l)
    top = u8[lay["top" + k]: lay["top" + k] + slots * 4].cpu().numpy().view(np.int32)
    cb = u8[lay["cb" + k]: lay["cb" + k] + slots * cbw * 8].cpu().numpy().view(np.uint64).reshape(slots, cbw)
    return dig, top, cb


@pytest.mark.parametrize("depth,w,L", STAGE_SHAPES + [(6, 512, 32760)], ids=STAGE_IDS + ["d6-w512-L32760"])
def test_weight_and_columns_stage(mp, torch_dev, depth, w, L):
    """MPFFT_STAGE_FWD_COLUMNS (split + weight launch, then the column DIF on slots) on a = 2^B (the
    top limb alone: x_0 = -1) and a random b: slot (p, c) of each operand == the model's column
    transform of theta^j x_j.  The workspace starts as 0xFF bytes."""
    import torch
    P = mp.mulmod_plan_info(L, depth, w)
    S = sm.Shape(P, depth, w)
    n2, b1, N, B = 2 * S.n, P["bits1"], S.N, 64 * L
    a, b = _limbs(1 << B, L), mp.fill_random(L + 1, 0x600 + w)
    b[L] = 0
    ws = mp.alloc_workspace_mulmod(L, depth, w, False, torch_dev)
    ws.fill_(0xFF)
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    mp.mulmod_stage(mp.STAGE_FWD_COLUMNS, da, db, dr, L, depth, w, ws)
    bad = []
    for which, v in ((0, to_int(a)), (1, to_int(b))):
        x = [(v >> (j * b1)) & ((1 << b1) - 1) for j in range(n2)]
        x[0] -= v >> B
        U = sm.fwd_columns([_theta(xj, j, w, N) for j, xj in enumerate(x)], S)
        dig, top, cb = _read_slots(mp, ws, L, depth, w, which)
        for pp in range(S.NR):
            for c in range(S.NC):
                s = pp * S.NC + c
                if sm.unpack_value(dig[s], top[s], cb[s], N) % S.p != U[pp][c]:
                    bad.append((which, pp, c))
    assert not bad, f"{len(bad)} slots wrong, first {bad[:6]}"


@pytest.mark.parametrize("depth,w,L", STAGE_SHAPES, ids=STAGE_IDS)
def test_unweight_stage_on_placed_slots(mp, torch_dev, depth, w, L):
    """slot j = theta^j 2^(depth+1) c_j in reduced form (carry limb in {-1, 0, 1}, +-1 carries on
    limbs), MPFFT_STAGE_SCALE: slot j must be the canonical residue of c_j"""
    import torch
    P = mp.mulmod_plan_info(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N = P["n"] * w
    p = (1 << N) + 1
    cmax = (1 << (2 * b1 + depth + 1)) - 1
    rng = random.Random(700 + depth + w)
    fixed = [0, 1, -1, cmax, -cmax]
    cs = [fixed[j % 8] if j % 8 < 5 else rng.randint(-cmax, cmax) for j in range(n2)]
    assert n2 >= 2 * len(sm.STYLES)
    ws = mp.alloc_workspace_mulmod(L, depth, w, False, torch_dev)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for shift in (0, 3):   # every value class meets several encodings
        ws.fill_(0x5A)
        enc = [sm.encode_reduced(_theta(c, j, w, N, depth + 1), (j // 8 + j + shift) % len(sm.STYLES), l, N, rng)
               for j, c in enumerate(cs)]
        dig, top, cb = _place(mp, torch_dev, ws, L, depth, w, enc)
        mp.mulmod_stage(mp.STAGE_SCALE, dr, dr, dr, L, depth, w, ws)
        torch.cuda.synchronize()
        hd, ht, hc = dig.cpu().numpy().view(np.uint64), top.cpu().numpy(), cb.cpu().numpy()
        bad = []
        for j, c in enumerate(cs):
            canon = not hc[j].any() and (ht[j] == 0 or (ht[j] == 1 and not hd[j].any()))
            if not canon or to_int(hd[j]) + (int(ht[j]) << N) != c % p:
                bad.append((j, c if abs(c) < 2 else "big", canon))
        assert not bad, f"{len(bad)} of {n2} slots wrong, first {bad[:6]}"


def _combine_patterns(n2, b1, depth, B, rng):
    cmax = (1 << (2 * b1 + depth + 1)) - 1
    z = [0] * n2
    t = rng.getrandbits(b1 + depth) | 1
    return [("all -1", [-1] * n2),
            ("alternating +-max", [cmax if j % 2 == 0 else -cmax for j in range(n2)]),
            ("alternating -+max", [-cmax if j % 2 == 0 else cmax for j in range(n2)]),
            ("last +max", z[:-1] + [cmax]),
            ("last -max", z[:-1] + [-cmax]),
            ("c_0 = -1: 2^B", [-1] + z[1:]),
            ("c_0 = -2: 2^B - 1, a borrow through every limb", [-2] + z[1:]),
            ("2^(B-1) - 1: the borrow stops in the last limb", [-1] + z[1:-1] + [1 << (b1 - 1)]),
            ("sum 0", [t << b1, -t] + z[2:]),
            ("sum 0 across the wrap", [t] + z[1:-1] + [t << b1]),
            ("all +max", [cmax] * n2),
            ("random", [rng.randint(-cmax, cmax) for _ in range(n2)]),
            ("zero", z)]


@pytest.mark.parametrize("depth,w,L", STAGE_SHAPES + [(4, 4, 7), (6, 64, 2048)],
                         ids=STAGE_IDS + ["d4-w4-L7", "d6-w64-L2048"])
def test_combine_stage_on_placed_coefficients(mp, torch_dev, depth, w, L):
    """canonical residues of signed c_j placed, MPFFT_STAGE_COMBINE: r == sum c_j 2^(j bits1) mod M,
    fully reduced (the workspace's flags and scratch start as 0x5A bytes)"""
    import torch
    P = mp.mulmod_plan_info(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N, B = P["n"] * w, 64 * L
    p = (1 << N) + 1
    rng = random.Random(900 + depth + w)
    ws = mp.alloc_workspace_mulmod(L, depth, w, False, torch_dev)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for name, cs in _combine_patterns(n2, b1, depth, B, rng):
        ws.fill_(0x5A)
        dr.fill_(0x5A5A)
        enc = []
        for c in cs:
            v = c % p
            enc.append((from_int(v & ((1 << N) - 1), l), (), (), v >> N))
        _place(mp, torch_dev, ws, L, depth, w, enc)
        mp.mulmod_stage(mp.STAGE_COMBINE, dr, dr, dr, L, depth, w, ws)
        torch.cuda.synchronize()
        want = sm.modp(sum(c << (j * b1) for j, c in enumerate(cs)), B)
        got = dr.cpu().numpy().view(np.uint64)
        assert to_int(got) == want, (depth, w, L, name)
        if name.startswith("c_0 = -1"):
            assert want == 1 << B and got[L] == 1
        if name.startswith("sum 0"):
            assert want == 0


def test_stage_entry_rejects_the_multiply_only_stages(mp, torch_dev):
    import torch
    depth, w, L = 6, 64, 4088
    ws = mp.alloc_workspace_mulmod(L, depth, w, False, torch_dev)
    d = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for stage in (mp.STAGE_FOLD_COMBINE, mp.STAGE_SCALE | mp.STAGE_DRIVEN, mp.STAGE_INV_ROWS | mp.STAGE_DRIVEN):
        with pytest.raises(mp.MpfftError) as e:
            mp.mulmod_stage(stage, d, d, d, L, depth, w, ws)
        assert e.value.code == 1


@pytest.mark.parametrize("L", [1, 14, 1000, 100000])
def test_host_entries(mp, oracle, L):
    """mulmod / sqrmod on host arrays at mulmod_choose's pair; a non-reduced operand is refused"""
    depth, w = mp.mulmod_choose(L)
    a, b = mp.fill_random(L + 1, 0xa0 + L), mp.fill_random(L + 1, 0xb0 + L)
    a[L] = b[L] = 0
    assert to_int(mp.mulmod(a, b, depth, w)) == _expected(oracle, a, b, L), (L, depth, w)
    assert to_int(mp.sqrmod(a, depth, w)) == _expected(oracle, a, a, L), (L, depth, w)
    top = _limbs(1 << (64 * L), L)
    assert to_int(mp.mulmod(top, top, depth, w)) == 1
    bad = a.copy()
    bad[L] = 1   # above 2^B
    for args in ((bad, b), (a, bad)):
        with pytest.raises(mp.MpfftError) as e:
            mp.mulmod(*args, depth, w)
        assert e.value.code == 1
    bad[L] = 2
    bad[:L] = 0
    with pytest.raises(mp.MpfftError):
        mp.sqrmod(bad, depth, w)


def test_next_size_product(mp, oracle):
    L, depth, w = mp.mulmod_next_size(5000)
    a, b = mp.fill_random(L + 1, 1), mp.fill_random(L + 1, 2)
    a[L] = b[L] = 0
    assert to_int(mp.mulmod(a, b, depth, w)) == _expected(oracle, a, b, L)


def test_profile_covers_mulmod(mp, torch_dev):
    import torch
    depth, w, L = 6, 512, 32760
    a = mp.fill_random(L + 1, 0x321)
    a[L] = 0
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    ws = mp.alloc_workspace_mulmod(L, depth, w, True, torch_dev)
    mp.profile_begin(1)
    mp.sqrmod_device(dr, da, L, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == 1
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert to_int(dr.cpu().numpy().view(np.uint64)) == sm.modp(to_int(a) ** 2, 64 * L)


def test_c_caller_mulmod(mp):
    exe = os.path.join(HERE, "c_mulmod", "mulmod_caller")
    assert os.path.exists(exe), "tests/c_mulmod/mulmod_caller not built (run __graft_entry__.build())"
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
