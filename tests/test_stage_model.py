"""CPU checks of the stage-boundary model (tests/stage_model.py): its formulas against the direct
definition of the transform, its encodings, and the shape table of the adversarial stage tests
against the library's planner (plan_info, stage_kernels, inv_columns_schedule: no GPU)."""
import random

import pytest

import stage_model as sm
from helpers import revbin

# (depth, w, NC, Tr): 2n = NR NC slots, square and not, truncated and not
SMALL = [(3, 8, 4, None), (4, 4, 4, 5), (4, 12, 8, 3)]


def _rand_x(S, rng, live=None):
    live = 2 * S.n if live is None else live
    return [rng.getrandbits(S.N + 1) % S.p if j < live else 0 for j in range(2 * S.n)]


@pytest.mark.parametrize("depth,w,NC,Tr", SMALL)
def test_forward_formulas_compose_to_the_definition(depth, w, NC, Tr):
    S = sm.small_shape(depth, w, NC, Tr)
    rng = random.Random(depth * 100 + w)
    x = _rand_x(S, rng)
    X = sm.dft(x, S)
    got = sm.forward(x, S)
    assert len(got) == S.Tr
    for pp in range(S.Tr):
        for q in range(S.NC):
            assert got[pp][q] == X[revbin(pp, S.lbR) + S.NR * revbin(q, S.lbC)], (pp, q)
    # the definition itself: omega = 2^w has order 2n, and X_0 is the plain sum
    assert pow(2, w * 2 * S.n, S.p) == 1 and pow(2, w * S.n, S.p) == S.p - 1
    assert X[0] == sum(x) % S.p


@pytest.mark.parametrize("depth,w,NC,Tr", SMALL)
def test_inverse_formulas_invert_the_forward_ones(depth, w, NC, Tr):
    S = sm.small_shape(depth, w, NC, Tr)
    rng = random.Random(depth * 7 + w)
    x = _rand_x(S, rng, S.T)   # rows >= Tr zero: what the truncated inverse assumes
    U = sm.fwd_columns(x, S)
    V = sm.inv_rows(sm.fwd_rows(U, S), S)
    for pp in range(S.Tr):
        for c in range(S.NC):
            assert V[pp][c] == S.NC * U[pp][c] % S.p, (pp, c)
    # the inverse columns' contract: from all NR rows of colDFT(y), NR y by the direct inverse sum;
    # the kernels get rows p < Tr only and y[r] = 0 for r >= Tr (the same linear system)
    y = [x[r * S.NC: (r + 1) * S.NC] for r in range(S.Tr)]
    W = sm.col_dft(y, S, S.NR)
    assert W[: S.Tr] == U
    for r in range(S.NR):
        for c in range(S.NC):
            acc = sum(sm.shl(W[pp][c], -S.w * S.NC * r * revbin(pp, S.lbR), S.N) for pp in range(S.NR))
            assert acc % S.p == S.NR * x[r * S.NC + c] % S.p, (r, c)
    # scaling: NC NR = 2n = 2^(depth+1)
    for v in x[:4]:
        assert sm.scaled(S.NC * S.NR * v % S.p, S) == v


@pytest.mark.parametrize("l,N", [(1, 64), (1, 29), (48, 3072), (48, 3050), (1024, 65536), (1024, 65500)])
def test_encode_reduced_round_trips(l, N):
    rng = random.Random(l + N)
    p = (1 << N) + 1
    values = [0, 1, 2, (1 << N) - 1, 1 << N, p - 2, rng.getrandbits(N) % p, rng.getrandbits(N) % p]
    for style in sm.STYLES:
        for v in values:
            limbs, pos, neg, top = sm.encode_reduced(v, style, l, N, rng)
            assert len(limbs) == l and not (pos & neg) and -1 <= top <= 1, (style, v)
            assert all(0 <= m < l for m in pos | neg)
            assert sm.val_reduced(limbs, pos, neg, top, N) % p == v, (style, v)
            # the same through the workspace's mask words
            cbw = 2 * ((l + 63) // 64)
            assert sm.unpack_value(limbs, top, sm.pack_masks(pos, neg, cbw), N) == sm.val_reduced(limbs, pos, neg, top, N)
            if style == "canonical":
                assert not pos and not neg and top == (1 if v == 1 << N and N == 64 * l else 0)
    assert sm.STYLES.index("canonical") == 0 and len(set(sm.STYLES)) == len(sm.STYLES)
    if N == 64 * l:
        for limbs, pos, neg, top in sm.literal_patterns(l, N, rng):
            assert len(limbs) == l and not (pos & neg) and -1 <= top <= 1


def test_value_patterns():
    rng = random.Random(5)
    N = 128
    p = (1 << N) + 1
    for pat in sm.PATTERNS:
        for cnt in (2, 8, 10):
            for rep in range(4):
                v = sm.line_values(pat, cnt, N, rng, rep)
                assert len(v) == cnt and all(0 <= t < p for t in v), pat
    v = sm.line_values("pairs", 8, N, rng, 1)
    assert all(v[i] == v[i ^ 2] for i in range(8))
    v = sm.line_values("alternate", 8, N, rng)
    assert all((v[i] + v[i + 1]) % p == 0 for i in range(7))


@pytest.mark.parametrize("row", sm.TABLE, ids=[r["id"] for r in sm.TABLE])
def test_shape_table_row(mp, row):
    """every row of the adversarial tests' shape table is of its class: kernel family, l, truncation
    case, fold -- and the placements fit its live slots and drop no (value pattern, style) pair"""
    S = sm.check_row(mp, row)
    for nlines, cnt in ((S.Tr, S.NC), (S.NC, S.Tr)):   # rows for the row stages, columns for the column stages
        runs = sm.placements(nlines, cnt)
        for off, sh in runs:
            placed = sum(len(sty) for _, _, sty in sm.assignment(nlines, cnt, off, sh))
            assert placed == nlines * cnt <= S.T
        assert sm.pairs_placed(nlines, cnt) == sm.all_pairs(), (row["id"], nlines, cnt)
        assert len(runs) <= 16   # (the l = 1 truncated shape: 16 live slots per run)
    lo, hi = sm.dbl_rows(S)
    assert (lo, hi) == (0, 0) if row["case"] == "full" else 0 <= lo < hi <= S.NR // 2
