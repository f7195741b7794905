"""An exact model of every stage boundary of the single-GPU pipeline (DESIGN.md "stage boundary
contract"), in plain Python integers mod p = 2^N + 1, and the adversarial encodings and value
patterns the stage tests place by hand (tests/test_gpu_stage_adversarial.py; CPU checks of the
model itself in tests/test_stage_model.py).

Every transform below is a direct sum of shifted integers -- no butterfly network, no shared
structure with the kernels.  rb = helpers.revbin, slot (row p, column c) = p NC + c, omega = 2^w
(order 2n = NR NC):

  after FWD_COLUMNS   U[p][c] = sum_r x[r NC + c] 2^(w NC r rb(p, lbR))                  p < Tr
  after FWD_ROWS      X[p][q] = sum_c U[p][c] 2^(w c (rb(p, lbR) + NR rb(q, lbC)))
                              = X_{rb(p) + NR rb(q)},  X_k = sum_j x_j 2^(w j k)
  after INV_ROWS      V[p][c] = 2^(-w c rb(p, lbR)) sum_q Z[p][q] 2^(-w NR c rb(q, lbC))
                      (unnormalised: NC U on forward data)
  after INV_COLUMNS   slot (r, c) = NR y[r][c] for V = colDFT(y), y[r] = 0 for r >= Tr
  after SCALE         the canonical value of 2^-(depth+1) times that
"""
import numpy as np

from helpers import log2, revbin

MAX = (1 << 64) - 1


class Shape:
    """the derived sizes of one (n1, n2, depth, w) plan (from mpfft_plan_info)"""

    def __init__(self, P, depth, w):
        self.depth, self.w = depth, w
        self.n, self.l, self.NC, self.NR, self.T, self.bits1 = P["n"], P["l"], P["NC"], P["NR"], P["trunc"], P["bits1"]
        self.N = self.n * w
        self.p = (1 << self.N) + 1
        self.Tr = self.T // self.NC
        self.lbR, self.lbC = log2(self.NR), log2(self.NC)
        self.j1, self.j2 = P["j1"], P["j2"]


def small_shape(depth, w, NC, Tr=None):
    """a Shape without a library (model tests): 2n = 2^(depth+1) slots in NC columns"""
    n = 1 << depth
    NR = 2 * n // NC
    P = {"n": n, "l": (n * w + 63) // 64, "NC": NC, "NR": NR, "trunc": (NR if Tr is None else Tr) * NC,
         "bits1": (n * w - depth) // 2, "j1": 0, "j2": 0}
    return Shape(P, depth, w)


def shl(x, e, N):
    """x 2^e mod p up to sign and size (2^N == -1: shifts only, no modexp); e any integer"""
    e %= 2 * N
    return x << e if e < N else -(x << (e - N))


def modp(v, N):
    """v mod p by folding at 2^N == -1 (a plain % of a 2N-bit sum by p costs a quadratic division)"""
    sign = -1 if v < 0 else 1
    v = abs(v)
    mask = (1 << N) - 1
    while v.bit_length() > N + 8:
        hi = v >> N
        v = (v & mask) - hi
        if v < 0:
            sign, v = -sign, -v
    return sign * v % ((1 << N) + 1)


def dft(x, S):
    """X_k = sum_j x_j 2^(w j k), k < 2n: the definition"""
    out = []
    for k in range(2 * S.n):
        acc = 0
        for j, xj in enumerate(x):
            if xj:
                acc += shl(xj, S.w * j * k, S.N)
        out.append(modp(acc, S.N))
    return out


def fwd_columns(x, S, rows=None):
    """U[p][c], p < rows (default Tr), of the 2n slot values x (slot r NC + c)"""
    rows = S.Tr if rows is None else rows
    U = []
    for pp in range(rows):
        e = S.w * S.NC * revbin(pp, S.lbR)
        row = []
        for c in range(S.NC):
            acc = 0
            for r in range(S.NR):
                xv = x[r * S.NC + c]
                if xv:
                    acc += shl(xv, e * r, S.N)
            row.append(modp(acc, S.N))
        U.append(row)
    return U


def col_dft(y, S, rows=None):
    """fwd_columns of y[r][c] given for r < len(y) (zero above)"""
    x = [0] * (2 * S.n)
    for r, row in enumerate(y):
        x[r * S.NC: (r + 1) * S.NC] = row
    return fwd_columns(x, S, rows)


def fwd_rows(U, S):
    """X[p][q] of the rows U[p][.]"""
    X = []
    for pp, urow in enumerate(U):
        rp = revbin(pp, S.lbR)
        row = []
        for q in range(S.NC):
            e = S.w * (rp + S.NR * revbin(q, S.lbC))
            acc = 0
            for c, uv in enumerate(urow):
                if uv:
                    acc += shl(uv, e * c, S.N)
            row.append(modp(acc, S.N))
        X.append(row)
    return X


def inv_rows(Z, S):
    """V[p][c] of the rows Z[p][.] (unnormalised inverse of fwd_rows: V = NC U)"""
    V = []
    for pp, zrow in enumerate(Z):
        rp = revbin(pp, S.lbR)
        row = []
        for c in range(S.NC):
            acc = 0
            for q, zv in enumerate(zrow):
                if zv:
                    acc += shl(zv, -S.w * c * (rp + S.NR * revbin(q, S.lbC)), S.N)
            row.append(modp(acc, S.N))
        V.append(row)
    return V


def forward(x, S):
    """the whole forward transform of 2n slot values: X[p][q], p < Tr"""
    return fwd_rows(fwd_columns(x, S), S)


def scaled(v, S):
    """canonical 2^-(depth+1) v"""
    return modp(shl(v, -(S.depth + 1), S.N), S.N)


def dbl_rows(S):
    """rows whose top-level doubling the driven truncated inverse leaves undone (plan.hpp plan_dbl)"""
    if S.Tr == S.NR:
        return 0, 0
    h = S.NR // 2
    return (0, S.Tr) if S.Tr <= h else (S.Tr - h, h)


# ---------------------------------------------------------------------------
# reduced-form encodings
# ---------------------------------------------------------------------------
# A slot holds l limbs, a +1 and a -1 carry per limb (limb m's lands at 2^(64 (m + 1)); limb l - 1's
# is the 2^N position when N = 64 l) and the carry limb `top` (weight 2^N).  Every style fixes the
# carries and the carry limb and solves the limbs for the value, so the limbs of small values (0,
# 1, 2^N) come out as the long all-ones / all-zero runs the carries then ripple through.  `top`
# stays within {-1, 0, 1}: no producing store emits more (stage boundary contract);
# v +- 2p uses the carry limb and limb l - 1's carry together.
STYLES = ("canonical", "plus_all", "minus_all", "chain_plus", "chain_minus", "top_plus", "top_minus",
          "top2_plus", "top2_minus", "sparse", "carry_top")
NONCANON = STYLES[1:]


def _boundaries(l):
    return sorted({max(0, k * l // 8 - 4) for k in range(1, 8)} & set(range(l)))


def _carry_int(ms, l):
    """sum over m in ms of 2^(64 (m + 1))"""
    if not ms:
        return 0
    a = np.zeros(l, np.uint64)
    a[list(ms)] = 1
    return int.from_bytes(a.tobytes(), "little") << 64


def val_reduced(limbs, pos, neg, top, N):
    """the value of an encoding (limbs: uint64 array; pos, neg: sets of limb indices)"""
    l = len(limbs)
    v = int.from_bytes(np.ascontiguousarray(limbs, dtype=np.uint64).tobytes(), "little") + top * (1 << N)
    return v + _carry_int(pos, l) - _carry_int(neg, l)


def encode_reduced(v, style, l, N, rng):
    """(limbs, pos, neg, top) with val_reduced(...) % p == v % p, in encoding `style` (a name of
    STYLES or its index); limbs a uint64 array of l, pos / neg disjoint sets, top in {-1, 0, 1}"""
    if not isinstance(style, str):
        style = STYLES[style % len(STYLES)]
    p = (1 << N) + 1
    assert 64 * (l - 1) < N <= 64 * l
    pos, neg, top = set(), set(), 0
    if style == "plus_all":
        pos = set(range(l))
    elif style == "minus_all":
        neg = set(range(l))
    elif style == "chain_plus":
        pos = set(_boundaries(l))
    elif style == "chain_minus":
        neg = set(_boundaries(l))
    elif style == "top_plus":
        top = 1
    elif style == "top_minus":
        top = -1
    elif style == "top2_plus":
        top, pos = 1, {l - 1}
    elif style == "top2_minus":
        top, neg = -1, {l - 1}
    elif style == "sparse":
        ms = rng.sample(range(l), min(l, 40))
        pos, neg = set(ms[: len(ms) // 2]), set(ms[len(ms) // 2:])
        top = rng.randint(-1, 1)
    elif style == "carry_top":
        pos = {l - 1}
    else:
        assert style == "canonical", style
    R = (v - val_reduced(np.zeros(l, np.uint64), pos, neg, top, N)) % p
    if R >> (64 * l):   # exactly 2^N = 2^(64 l): into the carry limb, or limb l - 1's carry
        R = 0
        if top < 1:
            top += 1
        elif l - 1 in neg:
            neg.discard(l - 1)
        else:
            assert l - 1 not in pos
            pos.add(l - 1)
    limbs = np.frombuffer(R.to_bytes(8 * l, "little"), dtype=np.uint64).copy()
    return limbs, pos, neg, top


def literal_patterns(l, N, rng):
    """hand-made encodings whose limbs are the pattern (test_gpu_parity._reduced_pattern's and
    test_gpu_fold._wrap_pattern's, the carry limb kept within {-1, 0, 1}): every limb all-ones with
    +1 on every limb, zeros with -1 on every limb, chains starting just below each k l / 8,
    2^N - 1, 2^N in the carry limb and in limb l - 1's carry, values at and next to m p"""
    out = [(np.full(l, MAX, np.uint64), set(range(l)), set(), 0),
           (np.zeros(l, np.uint64), set(), set(range(l)), 0),
           (np.full(l, MAX, np.uint64), set(range(l)), set(), 1),
           (np.zeros(l, np.uint64), set(), set(range(l)), -1),
           (np.full(l, MAX, np.uint64), set(), set(), 0),
           (np.zeros(l, np.uint64), set(), set(), 1),
           (np.zeros(l, np.uint64), {l - 1}, set(), 0)]
    limbs = np.array([rng.getrandbits(64) for _ in range(l)], dtype=np.uint64)
    for b in _boundaries(l):
        limbs[b + 1: b + 7] = MAX
    out.append((limbs, set(_boundaries(l)), set(), 0))
    out.append((np.zeros(l, np.uint64), set(), set(_boundaries(l)), 1))
    p = (1 << N) + 1
    for m in (-1, 0, 1):
        for d in (-1, 0, 1):
            v = m * p + d
            top = v >> N
            if N == 64 * l and -1 <= top <= 1:
                low = v - (top << N)
                out.append((np.frombuffer(low.to_bytes(8 * l, "little"), dtype=np.uint64).copy(), set(), set(), top))
    return out


# ---------------------------------------------------------------------------
# value patterns along one line (a row for the row stages, a column for the column stages)
# ---------------------------------------------------------------------------
# ("literal": the values of literal_patterns(); where the tested stage's input is free, the slot holds
# the literal encoding itself instead of a style's)
PATTERNS = ("eq_1", "eq_2N", "eq_2N-1", "eq_rand", "delta_0", "delta_last", "alternate", "pairs", "zeros",
            "top_piece", "x80", "random", "literal")


def line_values(pattern, cnt, N, rng, rep=0):
    """cnt residues mod p in value pattern `pattern`; `rep` (the pattern's repetition number) picks
    the butterfly distance of "pairs" (x[i] = x[i ^ h], h = 1, 2, 4, .. in turn)"""
    p = (1 << N) + 1
    rnd = lambda: rng.getrandbits(N + 1) % p   # noqa: E731
    if pattern == "eq_1":
        return [1] * cnt
    if pattern == "eq_2N":
        return [1 << N] * cnt
    if pattern == "eq_2N-1":
        return [(1 << N) - 1] * cnt
    if pattern == "eq_rand":
        return [rnd()] * cnt
    if pattern == "delta_0":
        return [rnd()] + [0] * (cnt - 1)
    if pattern == "delta_last":
        return [0] * (cnt - 1) + [rnd()]
    if pattern == "alternate":
        v = rnd()
        return [v if i % 2 == 0 else (p - v) % p for i in range(cnt)]
    if pattern == "pairs":
        nh = max(1, log2(cnt))
        h = 1 << (rep % nh)
        base = [rnd() for _ in range(cnt)]
        return [base[min(i, i ^ h) if (i ^ h) < cnt else i] for i in range(cnt)]
    if pattern == "zeros":
        return [0] * cnt
    if pattern == "top_piece":   # only the top limb's bits (and, every other slot, 2^N itself)
        return [(rng.getrandbits(64) << max(0, N - 64)) % p if i % 2 == 0 else 1 << N for i in range(cnt)]
    if pattern == "x80":
        return [int.from_bytes(b"\x80" * ((N + 7) // 8), "little") % p] * cnt
    if pattern == "literal" and N % 64 == 0:
        lits = literal_patterns(N // 64, N, rng)
        return [val_reduced(*lits[(j + rep * cnt) % len(lits)], N) % p for j in range(cnt)]
    assert pattern in ("random", "literal"), pattern
    return [rnd() for _ in range(cnt)]


def literal_encoding(v, l, N, rng):
    """the literal pattern whose value is v (a "literal" line's), None if there is none"""
    for e in literal_patterns(l, N, rng):
        if val_reduced(*e, N) % ((1 << N) + 1) == v:
            return e
    return None


def assignment(nlines, cnt, offset=0, sshift=0):
    """(pattern, rep, styles) per line: line i takes pattern (i + offset) mod |PATTERNS|; its slot j
    takes style (j + rep cnt + sshift) mod |STYLES|, rep counting the pattern's earlier lines.
    "zeros" takes only the non-canonical styles."""
    NP = len(PATTERNS)
    out = []
    for i in range(nlines):
        k = i + offset
        pat, rep = PATTERNS[k % NP], k // NP
        pool = NONCANON if pat == "zeros" else STYLES
        out.append((pat, rep, [pool[(j + rep * cnt + sshift) % len(pool)] for j in range(cnt)]))
    return out


def placements(nlines, cnt):
    """the (offset, sshift) runs of assignment() a test makes so that every value pattern meets
    every encoding style: the offsets give every pattern a line, the style shifts walk a line's cnt
    slots through all the styles"""
    offs = range(0, len(PATTERNS), nlines) if nlines < len(PATTERNS) else (0,)
    shifts = range(0, len(STYLES), cnt) if cnt < len(STYLES) else (0,)
    return [(o, s) for o in offs for s in shifts]


def pairs_placed(nlines, cnt):
    """the set of (pattern, style) pairs placements() places"""
    s = set()
    for off, sh in placements(nlines, cnt):
        for pat, _, sty in assignment(nlines, cnt, off, sh):
            s.update((pat, t) for t in sty if pat != "literal")
    return s


def all_pairs():
    return {(pat, t) for pat in PATTERNS if pat != "literal" for t in (NONCANON if pat == "zeros" else STYLES)}


# The shape table of the adversarial stage tests: the smallest shape of each class (depth, w,
# n1 = n2; None: the largest operands that fit).  family: the pass kernel; case: truncation case a
# (Tr <= NR / 2), b (NR / 2 < Tr < NR) or "full" (Tr == NR); fold: the reduced-form combine.
TABLE = [
    dict(id="wave-l1-trunc", depth=6, w=1, n=3, family="k_lpass", l=1, case="a", fold=False),
    dict(id="wave-l1-full", depth=6, w=1, n=None, family="k_lpass", l=1, case="full", fold=False),
    dict(id="wave-l48", depth=10, w=3, n=300, family="k_lpass", l=48, case="a", fold=False),
    dict(id="wave-l128", depth=9, w=16, n=2000, family="k_lpass", l=128, case="a", fold=False),
    dict(id="wave-l256", depth=8, w=64, n=3000, family="k_lpass", l=256, case="a", fold=False),
    dict(id="pass-l384", depth=8, w=96, n=4000, family="k_pass", l=384, case="a", fold=False),
    dict(id="bpass-l512", depth=7, w=256, n=4000, family="k_bpass", l=512, case="a", fold=False),
    dict(id="rpass-l1024-b", depth=7, w=512, n=33419, family="k_rpass", l=1024, case="b", fold=True,
         sched=("halfadd", "k_rchain", ",10> ")),      # FILL + half-add, k_rchain, the twiddle on load (mode bit 3)
    dict(id="rpass-l1024-a", depth=8, w=256, n=40000, family="k_rpass", l=1024, case="a", fold=True),
    dict(id="rpass-l2048-b", depth=7, w=1024, n=66842, family="k_rpass", l=2048, case="b", fold=True,
         NC=16),                                        # the doubled-column split: NC = 2^(depth/2 + 1)
    dict(id="rpass-l2048-a", depth=8, w=512, n=40000, family="k_rpass", l=2048, case="a", fold=True),
    dict(id="rpass-l4096-fold", depth=7, w=2048, n=133689, family="k_rpass", l=4096, case="b", fold=True,
         nosched=(",10> ", ",14> ")),                   # fold without the twiddle on load
    dict(id="rpass-l4096-full", depth=6, w=4096, n=100000, family="k_rpass", l=4096, case="full", fold=False),
]


def table_n(row):
    from helpers import max_limbs
    return row["n"] if row["n"] is not None else max_limbs(row["depth"], row["w"])


def check_row(mp, row):
    """asserts the class of a TABLE row against the library's planner (no GPU); returns its Shape"""
    d, w, n = row["depth"], row["w"], table_n(row)
    S = Shape(mp.plan_info(n, n, d, w), d, w)
    K = mp.stage_kernels(n, n, d, w)
    sched = "\n".join(mp.inv_columns_schedule(n, n, d, w)) + "\n"
    for st in ("fwd_columns", "fwd_rows", "inv_rows", "inv_columns"):
        assert K[st].startswith(row["family"]), (row["id"], st, K[st])
    assert S.l == row["l"], (row["id"], S.l)
    case = "full" if S.Tr == S.NR else "a" if S.Tr <= S.NR // 2 else "b"
    assert case == row["case"], (row["id"], S.Tr, S.NR)
    assert ("k_combine_red" in K["combine"]) == row["fold"], (row["id"], K["combine"])
    if "NC" in row:
        assert S.NC == row["NC"], (row["id"], S.NC)
    for word in row.get("sched", ()):
        assert word in sched, (row["id"], word, sched)
    for word in row.get("nosched", ()):
        assert word not in sched, (row["id"], word, sched)
    return S


# ---------------------------------------------------------------------------
# placing encodings into a workspace / reading slots back (GPU tests)
# ---------------------------------------------------------------------------
def pack_masks(pos, neg, cbw):
    """the cbw carry-mask words of a slot: word 2W / 2W + 1 bit k = limb 64 W + k carries +1 / -1"""
    out = np.zeros(cbw, np.uint64)
    for k, ms in ((0, pos), (1, neg)):
        if ms:
            bits = np.zeros(32 * cbw, np.uint8)
            bits[list(ms)] = 1
            out[k::2] = np.packbits(bits, bitorder="little").view(np.uint64)
    return out


def unpack_value(dig, top, cb, N):
    """the value of one slot as read back (dig: l limbs, cb: its mask words)"""
    l = len(dig)
    v = int.from_bytes(np.ascontiguousarray(dig).tobytes(), "little") + int(top) * (1 << N)
    if cb.any():
        for sign, words in ((1, cb[0::2]), (-1, cb[1::2])):
            bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:l]
            if bits.any():   # limb m's carry as limb m + 1 of a number
                v += sign * (int.from_bytes(bits.astype(np.uint64).tobytes(), "little") << 64)
    return v
