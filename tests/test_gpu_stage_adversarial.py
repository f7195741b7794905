"""Adversarial stage tests of the transform passes (k_lpass / k_wpass, k_pass / k_pairop, k_bpass,
k_rpass / k_rpair / k_rchain): hand-placed inputs at every stage boundary against the exact model
of tests/stage_model.py ("stage boundary contract").

Random operands reach the passes' rare carry, wrap and top branches with probability around
2^-32 per lane.  Here every live slot of a boundary is placed by hand: the value patterns
(stage_model.PATTERNS: all slots equal 1 / 2^N / 2^N - 1 / random, deltas, v and p - v alternating,
pairs equal at a butterfly distance, zeros, top-limb-only, 0x80 bytes, random) in the encodings
(stage_model.STYLES: canonical, +1 / -1 carries on every limb, chains across the k l / 8 segment
boundaries, v +- p and v +- 2p in the carry limb, sparse carries, limb l - 1's carry) and the
literal all-ones / all-zero chain patterns of the pointwise and scaling tests, every pattern meeting
every style.  One stage runs, and every slot it leaves must be the model's.  The workspace is
poisoned with 0x5A outside the placed slots.

The shape table (stage_model.TABLE) holds the smallest shape of each kernel class; every test first
asserts the class through the planner (stage_model.check_row), so a planner change cannot silently
move a case to another kernel.

test_inverse_driven runs the inverse stages as the whole multiply drives them
(MPFFT_STAGE_DRIVEN): the scaling riding in the last inverse row pass or, with the inverse MFA
twiddle, in the load of each column block's first pass, and the truncated inverse's top-level
doubling left to the scaling stage or to the folded combine.
"""
import random

import numpy as np
import pytest

import stage_model as sm
from helpers import chunks, to_int

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
ROWS = pytest.mark.parametrize("row", sm.TABLE, ids=[r["id"] for r in sm.TABLE])


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Bench:
    """one shape's workspace and the host side of its slots"""

    def __init__(self, mp, dev, row, n1=None, sqr=False):
        import torch
        self.mp, self.dev, self.row, self.sqr = mp, dev, row, sqr
        self.depth, self.w = row["depth"], row["w"]
        self.n2 = sm.table_n(row)
        self.n1 = self.n2 if n1 is None else n1
        if n1 is None:
            self.S = sm.check_row(mp, row)
        else:
            self.S = sm.Shape(mp.plan_info(self.n1, self.n2, self.depth, self.w), self.depth, self.w)
        a = (self.n1, self.n2, self.depth, self.w)
        self.kernels = mp.sqr_stage_kernels(self.n2, self.depth, self.w) if sqr else mp.stage_kernels(*a)
        self.lay = mp.sqr_workspace_layout(self.n2, self.depth, self.w) if sqr else mp.workspace_layout(*a)
        self.ws = mp.alloc_workspace_sqr(self.n2, self.depth, self.w, dev) if sqr else mp.alloc_workspace(*a, dev)
        self.da = torch.zeros(self.n1, dtype=torch.int64, device=dev)
        self.db = torch.zeros(self.n2, dtype=torch.int64, device=dev)
        self.dr = torch.zeros(self.n1 + self.n2, dtype=torch.int64, device=dev)
        self.poison()

    def poison(self):
        self.ws.fill_(0x5A)   # nothing may read a slot that was not placed or written

    def set_operands(self, a, b):
        import torch
        self.da = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(self.dev)
        self.db = torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint64).view(np.int64)).to(self.dev)

    def _regions(self, which):
        import torch
        k = "AB"[which]
        slots, l, cbw = self.lay["slots"], self.S.l, self.lay["cbw"]
        u8 = self.ws.view(torch.uint8)
        return (u8[self.lay["dig" + k]: self.lay["dig" + k] + slots * l * 8], u8[self.lay["top" + k]: self.lay["top" + k] + slots * 4],
                u8[self.lay["cb" + k]: self.lay["cb" + k] + slots * cbw * 8])

    def place(self, which, enc):
        """enc: slot -> (limbs, pos, neg, top); every other slot of the operand keeps the poison"""
        import torch
        slots, l, cbw = self.lay["slots"], self.S.l, self.lay["cbw"]
        dig = np.full((slots, l), 0x5A5A5A5A5A5A5A5A, np.uint64)
        top = np.full(slots, 0x5A5A5A5A, np.int32)
        cb = np.full((slots, cbw), 0x5A5A5A5A5A5A5A5A, np.uint64)
        for s, (limbs, pos, neg, t) in enc.items():
            dig[s] = limbs
            top[s] = t
            cb[s] = sm.pack_masks(pos, neg, cbw)
        for reg, arr in zip(self._regions(which), (dig, top, cb)):
            reg.copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)).to(self.dev))

    def read(self, which=0):
        import torch
        torch.cuda.synchronize()
        slots, l, cbw = self.lay["slots"], self.S.l, self.lay["cbw"]
        d, t, c = (r.cpu().numpy() for r in self._regions(which))
        return d.view(np.uint64).reshape(slots, l), t.view(np.int32), c.view(np.uint64).reshape(slots, cbw)

    def stage(self, which, flags=0):
        if self.sqr:
            self.mp.sqr_stage(which | flags, self.da, self.dr, self.n2, self.depth, self.w, self.ws)
        else:
            self.mp.stage(which | flags, self.da, self.db, self.dr, self.n1, self.n2, self.depth, self.w, self.ws)


def _hx(v):
    s = f"{v:x}"
    return s if len(s) <= 120 else s[:60] + ".." + s[-58:]


def _check(fails, B, name, got, want, info=None, canonical=False, exact=False):
    """got = B.read(); want: slot -> value mod p (exact: the slot's value itself, canonical form)"""
    S = B.S
    dig, top, cb = got
    for s in sorted(want):
        v = sm.unpack_value(dig[s], top[s], cb[s], S.N)
        tag = f"{name} [{B.row['id']}] slot ({s // S.NC},{s % S.NC})" + (f" pattern {info[s][0]} style {info[s][1]}" if info else "")
        if canonical or exact:
            t = int(top[s])
            if cb[s].any() or not (t == 0 or (t == 1 and not dig[s].any())):
                fails.append(f"{tag}: not canonical (top {t}, carry masks {'set' if cb[s].any() else 'zero'})")
        if (v if exact else v % S.p) != want[s]:
            fails.append(f"{tag}: got {_hx(v if exact else v % S.p)} (top {int(top[s])}) want {_hx(want[s])}")
        if len(fails) > 8:
            break
    return fails


def _lines(S, rng, nlines, cnt, off, sh):
    """one placement: (vals[line][j], styles[line][j], pattern name per line)"""
    vals, stys, names = [], [], []
    for pat, rep, sty in sm.assignment(nlines, cnt, off, sh):
        vals.append(sm.line_values(pat, cnt, S.N, rng, rep))
        stys.append(sty)
        names.append(pat)
    return vals, stys, names


def _place_values(B, which, rng, vals, stys, names, slot_of, literal=False):
    """encode vals[line][j] in style stys[line][j] into slot slot_of(line, j); literal: the slots of
    "literal" lines take the literal chain pattern their value comes from.  Returns info: slot -> (pattern, style)"""
    S = B.S
    enc, info = {}, {}
    for i, line in enumerate(vals):
        for j, v in enumerate(line):
            s = slot_of(i, j)
            e = sm.literal_encoding(v, S.l, S.N, rng) if literal and names[i] == "literal" else None
            if e is not None:
                enc[s], info[s] = e, (names[i], "literal")
            else:
                enc[s], info[s] = sm.encode_reduced(v, stys[i][j], S.l, S.N, rng), (names[i], stys[i][j])
    B.place(which, enc)
    return info


def _operands(mp, n1, n2, kind, seed):
    if kind == "random":
        return mp.fill_random(n1, seed), mp.fill_random(n2, seed + 1)
    if kind == "ones":
        return np.full(n1, MAX, np.uint64), np.full(n2, MAX, np.uint64)
    a, b = np.zeros(n1, np.uint64), np.zeros(n2, np.uint64)   # a single high bit
    a[n1 - 1] = 1 << 63
    b[n2 // 2] = 1 << 63
    return a, b


@ROWS
def test_fwd_columns_boundary(mp, torch_dev, row):
    """FWD_COLUMNS alone (split + truncated column DIF): every live slot of both operands == U, on
    operands that are random, all ones, a single high bit, and one limb against full length"""
    fails = []
    B = Bench(mp, torch_dev, row)
    cases = [(B, k) for k in ("random", "ones", "bit")]
    B1 = Bench(mp, torch_dev, row, n1=1)
    assert B1.kernels["fwd_columns"].split()[0] == B.kernels["fwd_columns"].split()[0]
    cases.append((B1, "ones"))
    for X, kind in cases:
        S = X.S
        a, b = _operands(mp, X.n1, X.n2, kind, 77 + S.l)
        X.poison()
        X.set_operands(a, b)
        X.stage(mp.STAGE_FWD_COLUMNS)
        for which, v in ((0, a), (1, b)):
            U = sm.fwd_columns(chunks(to_int(v), 2 * S.n, S.bits1), S)
            want = {pp * S.NC + c: U[pp][c] for pp in range(S.Tr) for c in range(S.NC)}
            _check(fails, X, f"fwd_columns {kind} n1={X.n1} op{which}", X.read(which), want)
    assert not fails, "\n".join(fails)


def _fwd_rows_placed(mp, dev, row, sqr):
    B = Bench(mp, dev, row, sqr=sqr)
    S = B.S
    canon = not B.kernels["pointwise"].startswith(("k_pwss", "k_pwsq"))   # those load the reduced form
    rng = random.Random(1000 + S.l + S.depth)
    fails = []
    for off, sh in sm.placements(S.Tr, S.NC):
        B.poison()
        placed = []
        for which in ((0,) if sqr else (0, 1)):   # operand B: other patterns against other styles
            vals, stys, names = _lines(S, rng, S.Tr, S.NC, off + 5 * which, sh + 3 * which)
            info = _place_values(B, which, rng, vals, stys, names, lambda i, j: i * S.NC + j, literal=True)
            placed.append((which, vals, info))
        B.stage(mp.STAGE_FWD_ROWS)
        for which, vals, info in placed:
            X = sm.fwd_rows(vals, S)
            want = {pp * S.NC + q: X[pp][q] for pp in range(S.Tr) for q in range(S.NC)}
            _check(fails, B, f"fwd_rows op{which}", B.read(which), want, info, canonical=canon)
        if fails:
            break
    assert not fails, "\n".join(fails)


@ROWS
def test_fwd_rows_placed(mp, torch_dev, row):
    """U placed on both operands, FWD_ROWS (MFA twiddle on load + row DIF): every slot == X, and
    canonical where the plan's pointwise family takes canonical input"""
    _fwd_rows_placed(mp, torch_dev, row, False)


def test_fwd_rows_placed_sqr(mp, torch_dev):
    """the same through mpfft_sqr_stage (operand 0 alone, the square's workspace layout)"""
    row = next(r for r in sm.TABLE if r["id"] == "rpass-l2048-b")
    assert mp.sqr_stage_kernels(sm.table_n(row), row["depth"], row["w"])["pointwise"].startswith("k_pwsq")
    _fwd_rows_placed(mp, torch_dev, row, True)


@ROWS
def test_inv_rows_placed(mp, torch_dev, row):
    """Z placed in the pointwise boundary's form (reduced, top in {-1, 0, 1}), INV_ROWS (row DIT +
    MFA un-twiddle): every slot == V"""
    B = Bench(mp, torch_dev, row)
    S = B.S
    rng = random.Random(2000 + S.l + S.depth)
    fails = []
    for off, sh in sm.placements(S.Tr, S.NC):
        B.poison()
        vals, stys, names = _lines(S, rng, S.Tr, S.NC, off, sh)
        info = _place_values(B, 0, rng, vals, stys, names, lambda i, j: i * S.NC + j, literal=True)
        B.stage(mp.STAGE_INV_ROWS)
        V = sm.inv_rows(vals, S)
        want = {pp * S.NC + c: V[pp][c] for pp in range(S.Tr) for c in range(S.NC)}
        if _check(fails, B, "inv_rows", B.read(), want, info):
            break
    assert not fails, "\n".join(fails)


@ROWS
def test_inv_columns_placed(mp, torch_dev, row):
    """y chosen per column from the value patterns (2^N and 2^N - 1 among them, which no product
    produces), colDFT(y) placed in adversarial encodings, INV_COLUMNS: slot (r, c) == NR y[r][c];
    then SCALE: canonical 2^-(depth+1) NR y.  Where the scaling is fused into the last inverse
    column pass (the untruncated wave plan), INV_COLUMNS already leaves that."""
    B = Bench(mp, torch_dev, row)
    S = B.S
    fused = B.kernels["scale"].startswith("(fused")
    assert fused == (row["id"] == "wave-l1-full")
    rng = random.Random(3000 + S.l + S.depth)
    fails = []
    for off, sh in sm.placements(S.NC, S.Tr):
        B.poison()
        ycol, stys, names = _lines(S, rng, S.NC, S.Tr, off, sh)   # ycol[c][r]
        y = [[ycol[c][r] for c in range(S.NC)] for r in range(S.Tr)]
        V = sm.col_dft(y, S)
        vals = [[V[pp][c] for pp in range(S.Tr)] for c in range(S.NC)]       # vals[c][p]: column lines
        _place_values(B, 0, rng, vals, stys, names, lambda c, pp: pp * S.NC + c)
        info = {r * S.NC + c: (names[c], stys[c][r]) for r in range(S.Tr) for c in range(S.NC)}
        B.stage(mp.STAGE_INV_COLUMNS)
        final = {r * S.NC + c: sm.scaled(S.NR * y[r][c] % S.p, S) for r in range(S.Tr) for c in range(S.NC)}
        if fused:
            _check(fails, B, "inv_columns (fused scale)", B.read(), final, info, exact=True)
        else:
            want = {r * S.NC + c: S.NR * y[r][c] % S.p for r in range(S.Tr) for c in range(S.NC)}
            _check(fails, B, "inv_columns", B.read(), want, info)
        B.stage(mp.STAGE_SCALE)
        _check(fails, B, "scale", B.read(), final, info, exact=True)
        if fails:
            break
    assert not fails, "\n".join(fails)


@ROWS
def test_inverse_driven(mp, torch_dev, row):
    """c[j], j < T, from the value patterns; Z = the model's forward transform of c placed in
    adversarial encodings; the inverse stages as the whole multiply drives them.  Fold plans: after
    driven INV_ROWS and INV_COLUMNS slot j == 2^(-s_j) c_j (s_j = 1 on the rows whose doubling is
    deferred), driven SCALE changes nothing, and FOLD_COMBINE of it is sum_j c_j 2^(j bits1).
    Other plans: after driven INV_ROWS, INV_COLUMNS, SCALE slot j is canonical and = c_j."""
    B = Bench(mp, torch_dev, row)
    S = B.S
    D = mp.STAGE_DRIVEN
    lo, hi = sm.dbl_rows(S)
    rng = random.Random(4000 + S.l + S.depth)
    fails = []
    for off, sh in sm.placements(S.Tr, S.NC):
        B.poison()
        cval, stys, names = _lines(S, rng, S.Tr, S.NC, off, sh)
        c = [v for line in cval for v in line]
        Z = sm.forward(c + [0] * (2 * S.n - S.T), S)
        _place_values(B, 0, rng, [list(r) for r in Z], stys, names, lambda i, j: i * S.NC + j)
        info = {s: (names[s // S.NC], stys[s // S.NC][s % S.NC]) for s in range(S.T)}
        B.stage(mp.STAGE_INV_ROWS, D)
        B.stage(mp.STAGE_INV_COLUMNS, D)
        if row["fold"]:
            want = {j: sm.modp(sm.shl(c[j], -(1 if lo <= j // S.NC < hi else 0), S.N), S.N) for j in range(S.T)}
            before = B.read()
            _check(fails, B, "driven inv_columns", before, want, info)
            B.stage(mp.STAGE_SCALE, D)
            after = B.read()
            if any((x != y).any() for x, y in zip(before, after)):
                fails.append(f"driven scale [{row['id']}]: changed a fold plan's slots")
            B.stage(mp.STAGE_FOLD_COMBINE)
            import torch
            torch.cuda.synchronize()
            total = B.n1 + B.n2
            L = S.j1 + S.j2 - 1
            prod = sum(c[j] << (j * S.bits1) for j in range(L)) & ((1 << (64 * total)) - 1)
            got = to_int(B.dr.cpu().numpy().view(np.uint64))
            if got != prod:
                x = got ^ prod
                fails.append(f"fold_combine [{row['id']}]: product differs, lowest wrong limb {((x & -x).bit_length() - 1) // 64} of {total}")
        else:
            B.stage(mp.STAGE_SCALE, D)
            _check(fails, B, "driven scale", B.read(), {j: c[j] for j in range(S.T)}, info, exact=True)
        if fails:
            break
    assert not fails, "\n".join(fails)
