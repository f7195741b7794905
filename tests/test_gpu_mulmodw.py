"""GPU tests of the products mod M = 2^B + 1 with the low-word CRT (mpfft_mulmodw_*):
whole products through every kernel family at pieces past the plain family's bound and at the
Fermat shapes, limb-equality with mpfft_mulmod_* where both are valid, the squaring entry, the
device-resident chain, the low-word convolution alone against the integer model, the fold alone on
hand-placed canonical slots and hand-placed low words, the host entries, profiling and a plain C
caller.  The reference is GMP (oracle.gmp_mul) or Python integers, folded at 2^B == -1; bit-exact is
the only bar.  Every whole-product test asserts the kernels of its shape first."""
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
from test_mulmodw_cpu import full_Lw, lowconv, pieces

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# tests/test_gpu_mulmod.py's (depth, w) list with L raised to this family's bound (its two shapes
# below full efficiency: (4, 4, 7) has bits1 = 14 < 32 and is left to the plain family, (6, 64, 2048)
# is valid in both), then the Fermat shapes at l = 1024, 2048 and 4096 (bits1 = N / 2).
# (depth, w, L, pointwise starts with, forward passes start with or None)
WHOLE = [
    (4, 4, 22, "k_pointwise", None),
    (4, 8, 38, "k_pointwise", None),
    (5, 64, 1036, "k_pw ", None),
    (6, 64, 4120, "k_pw ", ("k_lpass", "k_wpass")),
    (6, 64, 2048, "k_pw ", ("k_lpass", "k_wpass")),   # bits1 = N / 4: within the plain bound too
    (6, 128, 8216, "k_pwm ", None),
    (6, 192, 12312, "k_pw ", None),
    (6, 512, 32792, "k_pwm2", ("k_bpass",)),
    (5, 2048, 32780, "k_pwm2", ("k_rpass",)),
    (5, 4096, 65548, "k_pwss<18>", ("k_rpass",)),
    (6, 4096, 262168, "k_pwss<20>", ("k_rpass",)),
    (9, 256, 1048736, "k_pwss<18>", ("k_rpass",)),   # l = 2048, columns and rows in several passes each
    (8, 1024, 1048664, "k_pwss<20>", ("k_rpass",)),  # quad-fused pointwise at l = 4096, 512 slots
    (10, 128, 2097472, "k_pwss<18>", ("k_rpass",)),  # quad-fused pointwise at l = 2048, 2048 slots
    (6, 1, 88, "k_pointwise", None),           # odd w: theta = sqrt2
    (5, 2048, 32768, "k_pwm2", ("k_rpass",)),        # F: B = 2^21
    (5, 4096, 65536, "k_pwss<18>", ("k_rpass",)),    # F: B = 2^22
    (6, 4096, 262144, "k_pwss<20>", ("k_rpass",)),   # F: B = 2^24
]
PAIR, QUAD = "pair + last row level", "quad + last two row levels"
FUSED = {(6, 4096): PAIR, (9, 256): PAIR, (8, 1024): QUAD, (10, 128): QUAD}   # the later stages read C
WHOLE_IDS = ["d%d-w%d-L%d" % s[:3] for s in WHOLE]
BELOW = {(6, 64, 2048), (5, 2048, 32768), (5, 4096, 65536), (6, 4096, 262144)}   # not at the largest bits1
BOTH = [(6, 64, 2048), (6, 64, 4088), (4, 8, 30), (5, 2048, 32764), (5, 4096, 65532)]   # valid in both families


def _check_class(mp, depth, w, L, head, passes, sqr=False):
    assert mp.mulmodw_check_params(L, depth, w) == 0
    if (depth, w, L) not in BELOW:
        assert L == full_Lw(depth, w)
        assert mp.mulmod_check_params(L, depth, w) == 2   # MPFFT_ETOOBIG: past the plain bound
    sk = mp.mulmodw_stage_kernels(L, depth, w, sqr)
    pw = sk["pointwise"]
    if sqr and head.startswith("k_pwss"):
        head = head.replace("k_pwss", "k_pwsq")
    assert pw.startswith(head), (depth, w, L, pw)
    if sqr and not head.startswith("k_pwsq"):
        assert pw.endswith("(B = A)"), pw
    if passes:
        assert sk["inv_rows"].startswith(passes), sk
    assert sk["fwd_columns"].startswith("k_nweight<"), sk
    assert "k_nlowconv" in sk["combine"] and "k_nwrapw" in sk["combine"], sk
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
           ("2^B-1 squared", _limbs((1 << B) - 1, L), _limbs((1 << B) - 1, L)),   # |t| reaches 2n - 2
           ("M-2 squared", _limbs(M - 2, L), _limbs(M - 2, L)),
           ("2 times 2^(B-1)", _limbs(2, L), _limbs(1 << (B - 1), L)),
           ("one", _limbs(1, L), rb),
           ("zero", ra, _limbs(0, L)),
           ("top pieces", _limbs(rng.getrandbits(b1) << (top * b1), L), _limbs((rng.getrandbits(b1) | 1) << (top * b1), L))]
    if L % 2:
        f = (1 << 64) + 1
        assert M % f == 0
        out.append(("a factor times its cofactor", _limbs(f, L), _limbs(M // f, L)))
    return out


def _device(mp, dev, a, b, depth, w, L, ws=None, sqr=False, plain=False):
    import torch
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    dr = torch.full((L + 1,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    if ws is None:
        ws = (mp.alloc_workspace_mulmod if plain else mp.alloc_workspace_mulmodw)(L, depth, w, sqr, dev)
    ws.fill_(0xFF)   # no stage may rely on zeroed memory
    if sqr:
        (mp.sqrmod_device if plain else mp.sqrmodw_device)(dr, da, L, depth, w, ws)
    else:
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        (mp.mulmod_device if plain else mp.mulmodw_device)(dr, da, db, L, depth, w, ws)
    torch.cuda.synchronize()
    return dr.cpu().numpy().view(np.uint64)


def _whole(mp, oracle, dev, depth, w, L, head, passes):
    sk = _check_class(mp, depth, w, L, head, passes)
    B = 64 * L
    ws = mp.alloc_workspace_mulmodw(L, depth, w, False, dev)
    for name, a, b in _operands(mp, depth, w, L, 0x3000 + 17 * depth + w):
        got = _device(mp, dev, a, b, depth, w, L, ws)
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
    """mulmodw_device on every operand kind of _operands, one shape per kernel family"""
    sk = _whole(mp, oracle, torch_dev, depth, w, L, head, passes)
    if (depth, w) == (9, 256):   # more than one pass each way
        P = mp.mulmodw_plan_info(L, depth, w)
        assert P["NC"] >= 32 and P["NR"] >= 32, P
    if (depth, w) in FUSED:
        assert FUSED[(depth, w)] in sk["pointwise"], sk
    else:
        assert "pair" not in sk["pointwise"] and "quad" not in sk["pointwise"], sk


def test_whole_products_pwss_at_l1024(mp, torch_dev):
    """(5, 2048) through k_pwss<10>: MPFFT_POINTWISE=pwss in a fresh child process"""
    env = dict(os.environ, MPFFT_POINTWISE="pwss")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "5", "2048", "32780", "k_pwss<10>"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr


@pytest.mark.parametrize("depth,w,L", BOTH, ids=["d%d-w%d-L%d" % s for s in BOTH])
def test_limb_equal_to_the_plain_family_where_both_are_valid(mp, torch_dev, depth, w, L):
    assert mp.mulmod_check_params(L, depth, w) == 0 and mp.mulmodw_check_params(L, depth, w) == 0
    for name, a, b in _operands(mp, depth, w, L, 0x3500 + depth + w)[:5]:
        got = _device(mp, torch_dev, a, b, depth, w, L)
        want = _device(mp, torch_dev, a, b, depth, w, L, plain=True)
        assert (got == want).all(), (depth, w, L, name)
        assert (_device(mp, torch_dev, a, None, depth, w, L, sqr=True)
                == _device(mp, torch_dev, a, None, depth, w, L, sqr=True, plain=True)).all(), (depth, w, L, name)


@pytest.mark.parametrize("depth,w,L,head,passes", WHOLE, ids=WHOLE_IDS)
def test_sqrmodw(mp, oracle, torch_dev, depth, w, L, head, passes):
    """sqrmodw_device == mulmodw_device(a, a) == the exact value; k_pwsq on the nested plans"""
    sk = _check_class(mp, depth, w, L, head, passes, sqr=True)
    if head.startswith("k_pwss"):
        assert sk["pointwise"].startswith("k_pwsq"), sk
    for name, a, b in _operands(mp, depth, w, L, 0x4000 + 13 * depth + w)[:5]:
        if name == "2^B times random":
            a = b   # the random operand
        sq = _device(mp, torch_dev, a, None, depth, w, L, sqr=True)
        mu = _device(mp, torch_dev, a, a, depth, w, L)
        assert (sq == mu).all(), (depth, w, L, name)
        assert to_int(sq) == _expected(oracle, a, a, L), (depth, w, L, name)


@pytest.mark.parametrize("depth,w,L", [(6, 64, 4120), (5, 4096, 65536)])
def test_device_chain_of_squarings(mp, torch_dev, depth, w, L):
    """x -> x^2 three times on a non-default stream, two buffers ping-ponged, no host copy between
    (the result of one call is the operand of the next); the workspace starts as 0xFF bytes and
    nothing is written past it"""
    import torch
    B = 64 * L
    x = mp.fill_random(L + 1, 0x515)
    x[L] = 0
    nb = mp.mulmodw_workspace_bytes(L, depth, w, True)
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
        mp.sqrmodw_device(b1, b0, L, depth, w, ws, st)
        mp.sqrmodw_device(b0, b1, L, depth, w, ws, st)
        mp.sqrmodw_device(b1, b0, L, depth, w, ws, st)
    st.synchronize()
    want = to_int(x)
    for _ in range(3):
        want = sm.modp(want * want, B)
    assert to_int(b1.cpu().numpy().view(np.uint64)) == want
    assert torch.equal(buf[nb:], pat), "wrote past mpfft_mulmodw_workspace_bytes"
    EINVAL, ENOMEM = 1, 4
    lib = mp.lib()
    assert lib.mpfft_sqrmodw_device(b0.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb, None) == EINVAL
    assert lib.mpfft_sqrmodw_device(b1.data_ptr(), b0.data_ptr(), L, depth, w, ws.data_ptr(), nb - 1, None) == ENOMEM


# ---- MPFFT_STAGE_LOWCONV alone ------------------------------------------------------------------
# 2n = 8 (below any tile), 2n = 32 with bits1 = 76 (straddling limbs), 2n = 128 with bits1 = 32 (the
# words tile the operand), 2n = 2048 (two output tiles, the terms split over workgroups), 2n = 4096 with
# bits1 = 1000 (many tiles, bits1 no multiple of 32)
LOWCONV_SHAPES = [(2, 16, 5), (4, 8, 38), (6, 64, 64), (10, 2, 1024), (11, 1, 64000)]


def _lowconv_operands(mp, L, b1, n2):
    B = 64 * L
    ra, rb = mp.fill_random(L + 1, 0x771 + L), mp.fill_random(L + 1, 0x772 + L)
    ra[L] = rb[L] = 0
    ones = sum(0xFFFFFFFF << (j * b1) for j in range(n2))   # every low word all-ones, nothing else
    return [("random", ra, rb),
            ("2^B and random", _limbs(1 << B, L), rb),
            ("random and 2^B", ra, _limbs(1 << B, L)),
            ("2^B squared", _limbs(1 << B, L), _limbs(1 << B, L)),
            ("all-ones low words", _limbs(ones, L), _limbs(ones, L)),
            ("2^B - 1 and all-ones low words", _limbs((1 << B) - 1, L), _limbs(ones, L)),
            ("last piece and random", _limbs(0xFFFFFFFF << ((n2 - 1) * b1), L), rb)]


@pytest.mark.parametrize("depth,w,L", LOWCONV_SHAPES, ids=["d%d-w%d-L%d" % s for s in LOWCONV_SHAPES])
def test_lowconv_stage(mp, torch_dev, depth, w, L):
    """MPFFT_STAGE_LOWCONV: d == the negacyclic convolution mod 2^32 of the pieces' low words (the top
    limb in piece 0 as -1), on a multiply plan and, with one operand, on a squaring plan; d starts as
    0xFF bytes"""
    import torch
    P = mp.mulmodw_plan_info(L, depth, w)
    n2, b1, B = 2 * P["n"], P["bits1"], 64 * L
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for sqr in (False, True):
        ws = mp.alloc_workspace_mulmodw(L, depth, w, sqr, torch_dev)
        d = mp.mulmodw_workspace_views(ws, L, depth, w, sqr)[3]
        assert d.numel() == n2
        for name, a, b in _lowconv_operands(mp, L, b1, n2):
            if sqr:
                b = a
            ws.fill_(0xFF)
            da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
            db = torch.from_numpy(b.view(np.int64)).to(torch_dev)
            mp.mulmodw_stage(mp.STAGE_LOWCONV, da, da if sqr else db, dr, L, depth, w, ws, sqr)
            torch.cuda.synchronize()
            got = d.cpu().numpy().view(np.uint32)
            want = np.array(lowconv(pieces(to_int(a), B, n2, b1), pieces(to_int(b), B, n2, b1)), dtype=np.uint32)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (depth, w, L, name, sqr, bad[:6], got[bad[:6]], want[bad[:6]])
    with pytest.raises(mp.MpfftError) as e:   # the plain family has no such stage
        mp.mulmod_stage(mp.STAGE_LOWCONV, dr, dr, dr, 4088, 6, 64, mp.alloc_workspace_mulmod(4088, 6, 64, False, torch_dev))
    assert e.value.code == 1


# ---- MPFFT_STAGE_COMBINE alone ------------------------------------------------------------------
# the Fermat shape, an odd bits1, bits1 = 76 > N / 2, bits1 = 32 (neighbouring words touch), wave,
# register-pass and l = 4096 plans at the largest bits1, an odd w
COMBINE_SHAPES = [(4, 8, 32), (5, 4, 75), (4, 8, 38), (6, 64, 64), (6, 64, 4120), (5, 2048, 32780), (5, 4096, 65548),
                  (6, 4096, 262144), (6, 1, 88), (2, 16, 5)]


def _combine_patterns(n2, b1, N, rng):
    """(name, signed c_j) with floor(c_j / p) an int32: c~_j = c_j mod p and t_j = floor(c_j / p) are placed"""
    p = (1 << N) + 1
    z = [0] * n2
    ts = [-(1 << 31), (1 << 31) - 1, 0, -1]
    cts = [0, p - 1, 1, (1 << N) - 1]
    out = [("t=%d c~=%s everywhere" % (t, "0 p-1 1 2^N-1".split()[i]), [ct + t * p] * n2)
           for t in ts for i, ct in enumerate(cts)]
    combos = [ct + t * p for t in ts for ct in cts]
    big = rng.getrandbits(min(b1 + 20, N + 29 - b1)) | 1   # big 2^bits1 stays below 2^(N + 31)
    out += [("every extreme in turn", [combos[(j + j // 16) % 16] for j in range(n2)]),
            ("alternating extremes", [combos[1] if j % 2 else combos[7] for j in range(n2)]),
            ("last slot alone, t = -2^31, c~ = 2^N", z[:-1] + [combos[1]]),
            ("last slot alone, t = 2^31 - 1, c~ = 2^N", z[:-1] + [combos[5]]),
            ("c_0 = -1: 2^B", [-1] + z[1:]),
            ("c_0 = -2: 2^B - 1, a borrow through every limb", [-2] + z[1:]),
            ("2^(B-1) - 1: the borrow stops in the last limb", [-1] + z[1:-1] + [1 << (b1 - 1)]),
            ("sum 0", [big << b1, -big] + z[2:]),
            ("sum 0 across the wrap", [big] + z[1:-1] + [big << b1]),
            ("random", [rng.randrange(-(1 << (N + 31)) + 1, 1 << (N + 31)) for _ in range(n2)]),
            ("random small t", [rng.randrange(p) + rng.randint(-3, 3) * p for _ in range(n2)]),
            ("zero", z)]
    return out


@pytest.mark.parametrize("depth,w,L", COMBINE_SHAPES, ids=["d%d-w%d-L%d" % s for s in COMBINE_SHAPES])
def test_combine_stage_on_placed_coefficients_and_low_words(mp, torch_dev, depth, w, L):
    """canonical residues c~_j and low words d_j = c_j mod 2^32 placed, MPFFT_STAGE_COMBINE:
    r == sum (c~_j + t_j p) 2^(j bits1) mod M, fully reduced (flags and scratch start as 0x5A bytes)"""
    import torch
    P = mp.mulmodw_plan_info(L, depth, w)
    n2, l, b1 = 2 * P["n"], P["l"], P["bits1"]
    N, B = P["n"] * w, 64 * L
    p = (1 << N) + 1
    rng = random.Random(900 + depth + w)
    ws = mp.alloc_workspace_mulmodw(L, depth, w, False, torch_dev)
    dig, top, cb, d = mp.mulmodw_workspace_views(ws, L, depth, w)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for name, cs in _combine_patterns(n2, b1, N, rng):
        assert all(-(1 << 31) <= c // p < 1 << 31 for c in cs)   # t_j is an int32
        ws.fill_(0x5A)
        dr.fill_(0x5A5A)
        hd, ht = np.zeros((n2, l), np.uint64), np.zeros(n2, np.int32)
        for j, c in enumerate(cs):
            v = c % p
            hd[j], ht[j] = from_int(v & ((1 << N) - 1), l), v >> N
        dig.copy_(torch.from_numpy(hd.view(np.int64)).to(torch_dev))
        top.copy_(torch.from_numpy(ht).to(torch_dev))
        cb.zero_()
        d.copy_(torch.from_numpy(np.array([c % (1 << 32) for c in cs], dtype=np.uint32).view(np.int32)).to(torch_dev))
        mp.mulmodw_stage(mp.STAGE_COMBINE, dr, dr, dr, L, depth, w, ws)
        torch.cuda.synchronize()
        want = sm.modp(sum(c << (j * b1) for j, c in enumerate(cs)), B)
        got = dr.cpu().numpy().view(np.uint64)
        assert to_int(got) == want, (depth, w, L, name)
        assert got[L] == (1 if want == 1 << B else 0), (depth, w, L, name)
        if name.startswith("c_0 = -1"):
            assert want == 1 << B
        if name.startswith("c_0 = -2"):
            assert want == (1 << B) - 1
        if name.startswith("sum 0") or name == "zero":
            assert want == 0


def test_stage_entry_rejects_the_multiply_only_stages(mp, torch_dev):
    import torch
    depth, w, L = 6, 64, 4120
    ws = mp.alloc_workspace_mulmodw(L, depth, w, False, torch_dev)
    d = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    for stage in (mp.STAGE_FOLD_COMBINE, mp.STAGE_SCALE | mp.STAGE_DRIVEN, mp.STAGE_LOWCONV | mp.STAGE_DRIVEN):
        with pytest.raises(mp.MpfftError) as e:
            mp.mulmodw_stage(stage, d, d, d, L, depth, w, ws)
        assert e.value.code == 1


@pytest.mark.parametrize("L", [4, 38, 1000, 1 << 16])
def test_host_entries(mp, oracle, L):
    """mulmodw / sqrmodw on host arrays at mulmodw_choose's pair; a non-reduced operand is refused"""
    depth, w = mp.mulmodw_choose(L)
    a, b = mp.fill_random(L + 1, 0xa0 + L), mp.fill_random(L + 1, 0xb0 + L)
    a[L] = b[L] = 0
    assert to_int(mp.mulmodw(a, b, depth, w)) == _expected(oracle, a, b, L), (L, depth, w)
    assert to_int(mp.sqrmodw(a, depth, w)) == _expected(oracle, a, a, L), (L, depth, w)
    top = _limbs(1 << (64 * L), L)
    assert to_int(mp.mulmodw(top, top, depth, w)) == 1
    bad = a.copy()
    bad[L] = 1   # above 2^B
    for args in ((bad, b), (a, bad)):
        with pytest.raises(mp.MpfftError) as e:
            mp.mulmodw(*args, depth, w)
        assert e.value.code == 1
    bad[L] = 2
    bad[:L] = 0
    with pytest.raises(mp.MpfftError) as e:
        mp.sqrmodw(bad, depth, w)
    assert e.value.code == 1


def test_next_size_product(mp, oracle):
    L, depth, w = mp.mulmodw_next_size(5000)
    a, b = mp.fill_random(L + 1, 1), mp.fill_random(L + 1, 2)
    a[L] = b[L] = 0
    assert to_int(mp.mulmodw(a, b, depth, w)) == _expected(oracle, a, b, L)


def test_profile_covers_mulmodw(mp, torch_dev):
    """seven stage times; the low-word convolution runs between the un-weight's mark and the fold's,
    so the combine stage holds it (mulmodw_stage_kernels names it there)"""
    import torch
    depth, w, L = 6, 512, 32768
    assert "k_nlowconv" in mp.mulmodw_stage_kernels(L, depth, w, True)["combine"]
    a = mp.fill_random(L + 1, 0x321)
    a[L] = 0
    da = torch.from_numpy(a.view(np.int64)).to(torch_dev)
    dr = torch.zeros(L + 1, dtype=torch.int64, device=torch_dev)
    ws = mp.alloc_workspace_mulmodw(L, depth, w, True, torch_dev)
    mp.profile_begin(1)
    mp.sqrmodw_device(dr, da, L, depth, w, ws)
    ms, calls = mp.profile_end()
    assert calls == 1
    assert len(ms) == 7 and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
    assert ms["combine"] > 0, ms
    assert to_int(dr.cpu().numpy().view(np.uint64)) == sm.modp(to_int(a) ** 2, 64 * L)


def test_c_caller_mulmodw(mp):
    exe = os.path.join(HERE, "c_mulmodw", "mulmodw_caller")
    assert os.path.exists(exe), "tests/c_mulmodw/mulmodw_caller not built (run __graft_entry__.build())"
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
