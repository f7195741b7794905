"""Adversarial stage tests of the shard transform stages (mpfft_shard_stage, mpfft_shard_stage_rows):
the passes tests/test_gpu_stage_adversarial.py covers on the single-GPU layout, here in the shard
layouts -- the column layout with ccount < NC, the row layout with its block stride, own-rows
forward columns, sliced operands, the row phase in chunks, and INV_COLUMNS with the deferred
doubling followed by the scale -- on hand-placed inputs against the exact model of
tests/stage_model.py.  Every rank sits on device 0; `rowc` is NULL, so the row stages are the
complete, unfused ones the model describes.  Everything not placed holds the 0x5A poison.

Worlds: 2 on every stage_model.TABLE row, 4 where the partition accepts it (every row but
wave-l1-trunc and wave-l48; with a one-limb first operand only the rows of W4_N1).
"""
import random

import numpy as np
import pytest

import stage_model as sm
from helpers import chunks, to_int
from test_gpu_stage_adversarial import _check, _lines, _operands, _place_values

pytestmark = pytest.mark.gpu
NO_W4 = ("wave-l1-trunc", "wave-l48")
# the rows whose partition accepts four ranks when the first operand is one limb
W4_N1 = ("wave-l1-full", "rpass-l1024-b", "rpass-l1024-a", "rpass-l2048-b", "rpass-l2048-a", "rpass-l4096-fold",
         "rpass-l4096-full")
CASES = [(r, wd) for r in sm.TABLE for wd in (2, 4) if wd == 2 or r["id"] not in NO_W4]
RW = pytest.mark.parametrize("row,world", CASES, ids=[f"{r['id']}-w{wd}" for r, wd in CASES])
_MODEL = {}   # references shared by the worlds of a row


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cached(key, make):
    if key not in _MODEL:
        _MODEL[key] = make()
    return _MODEL[key]


class ShardBench:
    """one TABLE row split over `world` ranks: every rank's column and row arrays of both operands,
    and the natural slot (pos, c) = pos NC + c in either layout:
      column layout  rank c // C, slot pos C + c % C
      row layout     the rank d with r0 <= pos < r0 + rcount, slot (c / ccb) rcount ccb + (pos - r0) ccb + c % ccb
    (include/mpfft.h; ccb = C)"""

    def __init__(self, mp, dev, row, world, n1=None):
        import torch
        from mpir_fft_amd.sharded import GpuBackend, ShardPlan
        self.mp, self.dev, self.row, self.world, self.torch = mp, dev, row, world, torch
        self.depth, self.w = row["depth"], row["w"]
        self.n2 = sm.table_n(row)
        self.n1 = self.n2 if n1 is None else n1
        if n1 is None:
            self.S = sm.check_row(mp, row)
        else:
            self.S = sm.Shape(mp.plan_info(self.n1, self.n2, self.depth, self.w), self.depth, self.w)
        self.plan = p = ShardPlan(mp, self.n1, self.n2, self.depth, self.w, world)   # a rejected world raises
        assert (p.C, p.Tr, p.NC, p.l) == (self.S.NC // world, self.S.Tr, self.S.NC, self.S.l)
        assert p.rows[0] == 0 and p.rows[-1] == p.Tr
        be = GpuBackend(mp, p, dev)
        self.colarr = [[be.alloc_coeffs(p.col_slots()) for _ in range(2)] for _ in range(world)]
        self.rowarr = [[be.alloc_coeffs(p.row_slots(g)) for _ in range(2)] for g in range(world)]
        self.layout = "row"
        self.kernels = mp.stage_kernels(self.n1, self.n2, self.depth, self.w)
        self.last = {}
        self.poison()

    def desc(self, g, c0=None, src_chunk=0):
        p = self.plan
        return self.mp.shard_desc(dict(n1=p.n1, n2=p.n2, depth=p.depth, w=p.w, c0=g * p.C if c0 is None else c0,
                                       ccount=p.C, r0=p.rows[g], rcount=p.rcount(g), ccb=p.C, col=self.colarr[g],
                                       row=self.rowarr[g], src_chunk=src_chunk, rowc=None))

    def poison(self):
        t = self.torch
        for arrs in self.colarr + self.rowarr:
            for a in arrs:
                for f in a.values():
                    f.view(t.uint8).fill_(0x5A)

    # per-rank arrays <-> natural (Tr NC slots) arrays, field by field
    def _rank_view(self, layout, g, which, f, width):
        """rank g's array of field f as (rows, blocks or 1, C, width) with the natural row range it holds"""
        p = self.plan
        a = (self.colarr if layout == "col" else self.rowarr)[g][which][f]
        if layout == "col":
            return a.view(p.NR, 1, p.C, width)[: p.Tr], 0, p.Tr, slice(g, g + 1)
        return a.view(p.NC // p.C, p.rcount(g), p.C, width).permute(1, 0, 2, 3), p.rows[g], p.rows[g + 1], slice(None)

    def place(self, which, enc):
        """enc: natural slot -> (limbs, pos, neg, top) into the current layout; every other slot of the
        operand's arrays keeps the poison"""
        p, t = self.plan, self.torch
        self.last[which] = enc
        T, l, cbw = p.Tr * p.NC, p.l, p.cbw
        nat = {"dig": np.full((T, l), 0x5A5A5A5A5A5A5A5A, np.uint64), "cb": np.full((T, cbw), 0x5A5A5A5A5A5A5A5A, np.uint64),
               "top": np.full((T, 1), 0x5A5A5A5A, np.int32)}
        for s, (limbs, pos, neg, top) in enc.items():
            nat["dig"][s] = limbs
            nat["top"][s] = top
            nat["cb"][s] = sm.pack_masks(pos, neg, cbw)
        for g in range(self.world):
            for f, width in (("dig", l), ("cb", cbw), ("top", 1)):
                view, lo, hi, blocks = self._rank_view(self.layout, g, which, f, width)
                src = nat[f].reshape(p.Tr, self.world, p.C, width)[lo:hi, blocks]
                view.copy_(t.from_numpy(np.ascontiguousarray(src).view(np.int32 if f == "top" else np.int64)).to(self.dev))

    def read(self, which=0, block_ranks=None):
        """(dig, top, cb) by natural slot, as Bench.read.  block_ranks (column layout): row -> the
        rank whose arrays hold that row (own-rows forward columns), with the block they computed"""
        p, t = self.plan, self.torch
        t.cuda.synchronize()
        T, l, cbw = p.Tr * p.NC, p.l, p.cbw
        nat = {"dig": np.zeros((T, l), np.uint64), "cb": np.zeros((T, cbw), np.uint64), "top": np.zeros((T, 1), np.int32)}
        for g in range(self.world):
            for f, width in (("dig", l), ("cb", cbw), ("top", 1)):
                view, lo, hi, blocks = self._rank_view(self.layout, g, which, f, width)
                if block_ranks is not None:
                    lo, hi, blocks = p.rows[g], p.rows[g + 1], slice(block_ranks, block_ranks + 1)
                    view = view[lo:hi]
                arr = view.contiguous().cpu().numpy()
                nat[f].reshape(p.Tr, self.world, p.C, width)[lo:hi, blocks] = arr.view(np.int32 if f == "top" else np.uint64)
        return nat["dig"], nat["top"].reshape(-1), nat["cb"]

    def stage(self, which, d1=None, d2=None, src_chunk=0):
        for g in range(self.world):
            a, b = (d1[g], d2[g]) if isinstance(d1, list) else (d1, d2)
            self.mp.shard_stage(which, self.desc(g, src_chunk=src_chunk), a, b)

    def stage_chunked(self, which):
        """the row stage in two uneven chunks of local rows, [0, 1) and [1, rcount)"""
        for g in range(self.world):
            rc = self.plan.rcount(g)
            for lo, hi in ((0, 1), (1, rc)) if rc >= 2 else ((0, rc),):
                self.mp.shard_stage_rows(which, self.desc(g), lo, hi)


def _dev(B, a):
    return B.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(B.dev)


def _own_slices(B, a, g):
    """rank g's column slices of operand a for its own column block (mpfft_shard_pack lists every
    block's in turn where the forward columns are replicated)"""
    p = B.plan
    pack = B.mp.shard_pack(a, p.n1, p.n2, p.depth, p.w, p.world, g)
    per = p.Tr * p.chunk
    assert len(pack) in (per, p.world * per)
    return pack if len(pack) == per else pack[g * per: (g + 1) * per]


@RW
def test_shard_fwd_columns(mp, torch_dev, row, world):
    """FWD_COLUMNS in the column layout: stage 0, stages _A then _B, and _OWN (only rows
    [r0, r0 + rcount) of each block), on the whole operands and on the ranks' slices: every live
    slot of both operands == U.  Operands random, all ones, a single high bit, one limb against
    full length."""
    fails = []
    B = ShardBench(mp, torch_dev, row, world)
    B.layout = "col"
    cases = [(B, k) for k in ("random", "ones", "bit")]
    if world == 2 or row["id"] in W4_N1:
        cases.append((ShardBench(mp, torch_dev, row, world, n1=1), "ones"))
        cases[-1][0].layout = "col"
    else:
        with pytest.raises(mp.MpfftError):   # (the partition rejects it: nothing to run)
            mp.shard_partition(1, B.n2, B.depth, B.w, world)
    for X, kind in cases:
        S, p = X.S, X.plan
        a, b = _operands(mp, X.n1, X.n2, kind, 77 + S.l)
        want = []
        for which, v in ((0, a), (1, b)):
            U = _cached(("U", row["id"], X.n1, kind, which),
                        lambda: sm.fwd_columns(chunks(to_int(v), 2 * S.n, S.bits1), S))
            want.append({pp * S.NC + c: U[pp][c] for pp in range(S.Tr) for c in range(S.NC)})
        da, db = _dev(X, a), _dev(X, b)
        sa = [_dev(X, _own_slices(X, a, g)) for g in range(world)]
        sb = [_dev(X, _own_slices(X, b, g)) for g in range(world)]
        for name, stages, d1, d2, chunk in (("stage 0", (0,), da, db, 0), ("stages A, B", (5, 6), da, db, 0),
                                            ("stage 0 sliced", (0,), sa, sb, p.chunk),
                                            ("stages A, B sliced", (5, 6), sa, sb, p.chunk)):
            X.poison()
            for st in stages:
                X.stage(st, d1, d2, src_chunk=chunk)
            for which in (0, 1):
                _check(fails, X, f"fwd_columns {name} {kind} n1={X.n1} world {world} op{which}", X.read(which), want[which])
        for blk in range(world):   # own rows: every rank computes block blk for its rows
            X.poison()
            for g in range(world):
                mp.shard_stage(7, X.desc(g, c0=blk * p.C), da, db)
            for which in (0, 1):
                w_blk = {s: v for s, v in want[which].items() if (s % S.NC) // p.C == blk}
                _check(fails, X, f"fwd_columns own block {blk} {kind} n1={X.n1} world {world} op{which}",
                       X.read(which, block_ranks=blk), w_blk)
        if fails:
            break
    assert not fails, "\n".join(fails)


def _row_stage(mp, dev, row, world, stage, model, ops, seed, literal=True):
    B = ShardBench(mp, dev, row, world)
    S = B.S
    canon = stage == 1 and not B.kernels["pointwise"].startswith(("k_pwss", "k_pwsq"))
    fails = []
    for off, sh in sm.placements(S.Tr, S.NC):
        placed = []
        B.poison()
        for which in ops:
            def make(which=which):
                rng = random.Random(hash((seed, S.l, S.depth, which, off, sh)) & 0xFFFFFFFF)
                vals, stys, names = _lines(S, rng, S.Tr, S.NC, off + 5 * which, sh + 3 * which)
                M = model(vals, S)
                return vals, stys, names, {pp * S.NC + q: M[pp][q] for pp in range(S.Tr) for q in range(S.NC)}
            vals, stys, names, want = _cached((stage, row["id"], off, sh, which), make)
            rng = random.Random(seed + off * 31 + sh + which)
            info = _place_values(B, which, rng, vals, stys, names, lambda i, j: i * S.NC + j, literal=literal)
            placed.append((which, want, info))
        B.stage(stage)
        whole = [B.read(which) for which, _, _ in placed]
        encs = dict(B.last)
        B.poison()
        for which, enc in encs.items():
            B.place(which, enc)
        B.stage_chunked(stage)
        for (which, want, info), got in zip(placed, whole):
            _check(fails, B, f"stage {stage} world {world} op{which}", got, want, info, canonical=canon)
            again = B.read(which)
            if any((x != y).any() for x, y in zip(got, again)):
                fails.append(f"stage {stage} [{row['id']}] world {world} op{which}: the chunked run differs from the whole one")
        if fails:
            break
    assert not fails, "\n".join(fails)


@RW
def test_shard_fwd_rows(mp, torch_dev, row, world):
    """U placed on both operands in the row layout, FWD_ROWS through mpfft_shard_stage and again in
    two uneven row chunks through mpfft_shard_stage_rows: every slot == X both times, and the two
    runs agree slot for slot"""
    _row_stage(mp, torch_dev, row, world, 1, sm.fwd_rows, (0, 1), 1000)


@RW
def test_shard_inv_rows(mp, torch_dev, row, world):
    """Z placed in the row layout, INV_ROWS whole and in chunks: every slot == V"""
    _row_stage(mp, torch_dev, row, world, 3, sm.inv_rows, (0,), 2000)


@RW
def test_shard_inv_columns(mp, torch_dev, row, world):
    """colDFT(y) placed in the column layout in adversarial encodings, INV_COLUMNS (the truncated
    inverse with its doubling deferred, then the scale): every live slot canonical and
    == 2^-(depth+1) NR y[r][c]"""
    B = ShardBench(mp, torch_dev, row, world)
    B.layout = "col"
    S = B.S
    fails = []
    for off, sh in sm.placements(S.NC, S.Tr):
        def make():
            rng = random.Random(hash((3000, S.l, S.depth, off, sh)) & 0xFFFFFFFF)
            ycol, stys, names = _lines(S, rng, S.NC, S.Tr, off, sh)   # ycol[c][r]
            y = [[ycol[c][r] for c in range(S.NC)] for r in range(S.Tr)]
            V = sm.col_dft(y, S)
            vals = [[V[pp][c] for pp in range(S.Tr)] for c in range(S.NC)]
            final = {r * S.NC + c: sm.scaled(S.NR * y[r][c] % S.p, S) for r in range(S.Tr) for c in range(S.NC)}
            return vals, stys, names, final
        vals, stys, names, final = _cached((4, row["id"], off, sh), make)
        B.poison()
        rng = random.Random(3000 + off * 31 + sh)
        _place_values(B, 0, rng, vals, stys, names, lambda c, pp: pp * S.NC + c)
        info = {r * S.NC + c: (names[c], stys[c][r]) for r in range(S.Tr) for c in range(S.NC)}
        B.stage(4)
        if _check(fails, B, f"inv_columns world {world}", B.read(), final, info, exact=True):
            break
    assert not fails, "\n".join(fails)
