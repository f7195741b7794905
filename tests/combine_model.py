"""An exact model of the combine's stripe contract (csrc/combine.hpp, include/mpfft.h
mpfft_shard_combine) in plain Python integers, and the coefficient patterns the placed combine
tests run (tests/test_gpu_combine_placed.py; CPU checks of the model in tests/test_combine_model.py).

Coefficients 0 <= c_k < 2^N, k < len, term t_k = c_k 2^(k bits1).  The 64-bit window of
coefficient k at product limb m is win(k, m) = floor(t_k / 2^(64 m)) mod 2^64, and
lo_m + 2^64 hi_m = sum_k win(k, m).  Stripe s owns limbs [ms[s], ms[s+1]), n of them.  Its phase-0
value X_s is the carry chain, with carry-in 0, of v_m = lo_m + hi_(m-1) over its limbs: hi of the
limb just below the stripe counts to it, hi of its last limb does not (it belongs to the next
stripe).  With A(m) = sum_k floor(t_k / 2^(64 m)),

    X_s = A(ms) - (A(me) << 64 n) + hi(ms - 1) - (hi(me - 1) << 64 n)

and A(ms) - (A(me) << 64 n) = sum_k (floor(t_k / 2^(64 ms)) mod 2^(64 n)) term by term, which only
the coefficients reaching the stripe's limbs enter: that is what stripe_value() sums, so no number
longer than a stripe is ever formed (stripe_value_A() is the formula above as written, for the CPU
test).  From X_s: the stripe's limbs X_s mod 2^(64 n), generate = X_s >> 64 n (0 or 1), propagate
= every limb all-ones; an empty stripe gives (0, 1).  Chaining (generate, propagate) in product
order and adding each stripe's carry-in gives sum_k t_k mod 2^(64 total).
"""
import random

M64 = (1 << 64) - 1


class Contract:
    """one product's sizes and stripes: ms[0 .. S] the stripes' first limbs (ms[S] = total); stripe s
    belongs to rank s % world and starts at coefficient s C; H halo coefficients before it"""

    def __init__(self, N, bits1, length, total, ms, world=1, C=None, H=0):
        self.N, self.bits1, self.len, self.total = N, bits1, length, total
        self.ms, self.S, self.world = list(ms), len(ms) - 1, world
        self.C = C if C is not None else length
        self.H = H
        assert self.ms[0] == 0 and self.ms[-1] == total and all(a <= b for a, b in zip(ms, ms[1:]))

    def n(self, s):
        return self.ms[s + 1] - self.ms[s]

    def rank(self, s):
        return s % self.world

    def klo(self, m):
        """first coefficient reaching past bit 64 m"""
        return (64 * m - self.N) // self.bits1 + 1 if 64 * m >= self.N else 0

    def khi(self, m):
        """last coefficient starting below bit 64 m + 64"""
        return min((64 * m + 63) // self.bits1, self.len - 1)


def shard_contract(mp, n1, n2, depth, w, world):
    """the Contract of a column-sharded product, from the library's planner (no GPU)"""
    P = mp.plan_info(n1, n2, depth, w)
    part = mp.shard_partition(n1, n2, depth, w, world)
    K = Contract(P["n"] * w, P["bits1"], P["j1"] + P["j2"] - 1, n1 + n2, part["ms"], world, part["C"], part["H"])
    K.l, K.Tr, K.SL, K.NC = P["l"], part["Tr"], part["SL"], P["NC"]
    return K


def single_contract(N, bits1, length, total):
    return Contract(N, bits1, length, total, [0, total])


def sparse(c):
    """coefficients as {k: c_k != 0} (from a list or a dict)"""
    items = c.items() if isinstance(c, dict) else enumerate(c)
    return {k: v for k, v in items if v}


def check_range(K, c):
    for k, v in sparse(c).items():
        assert 0 <= k < K.len and 0 <= v < (1 << K.N), (k, K.len)


def _shift(v, sh):
    return v << sh if sh >= 0 else v >> -sh


def window_sum(K, c, m):
    """(lo_m, hi_m); (0, 0) below limb 0"""
    if m < 0:
        return 0, 0
    acc = 0
    for k in range(K.klo(m), K.khi(m) + 1):
        v = c.get(k)
        if v:
            acc += _shift(v, k * K.bits1 - 64 * m) & M64
    return acc & M64, acc >> 64


def A(K, c, m):
    """sum_k floor(t_k / 2^(64 m))"""
    return sum(_shift(v, k * K.bits1 - 64 * m) for k, v in c.items())


def _summary(K, s, X):
    n = K.n(s)
    if n == 0:
        return 0, 0, 1
    assert 0 <= X < (2 << (64 * n)), f"stripe {s}: carry out of phase 0 is not 0 or 1"
    limbs = X & ((1 << (64 * n)) - 1)
    return limbs, X >> (64 * n), int(limbs == (1 << (64 * n)) - 1)


def stripe_value(K, c, s):
    """(limbs as an integer, generate, propagate) of stripe s after phase 0"""
    c = sparse(c)
    m0, m1 = K.ms[s], K.ms[s + 1]
    n = m1 - m0
    if n == 0:
        return 0, 0, 1
    mask = (1 << (64 * n)) - 1
    X = 0
    for k in range(K.klo(m0), K.khi(m1 - 1) + 1):
        v = c.get(k)
        if v:
            X += _shift(v, k * K.bits1 - 64 * m0) & mask
    X += window_sum(K, c, m0 - 1)[1] - (window_sum(K, c, m1 - 1)[1] << (64 * n))
    return _summary(K, s, X)


def stripe_value_A(K, c, s):
    """the same from A(m) at the stripe's two boundaries"""
    c = sparse(c)
    m0, m1 = K.ms[s], K.ms[s + 1]
    n = m1 - m0
    X = A(K, c, m0) - (A(K, c, m1) << (64 * n)) + window_sum(K, c, m0 - 1)[1] - (window_sum(K, c, m1 - 1)[1] << (64 * n))
    return _summary(K, s, X)


def stripe_naive(K, c, s):
    """the same limb by limb: v_m = lo_m + hi_(m-1), carry chain with carry-in 0"""
    c = sparse(c)
    m0, m1 = K.ms[s], K.ms[s + 1]
    run, limbs, allp = 0, 0, 1
    hi_below = window_sum(K, c, m0 - 1)[1]
    for m in range(m0, m1):
        lo, hi = window_sum(K, c, m)
        v = lo + hi_below
        allp &= int(v == M64)
        t = v + run
        limbs |= (t & M64) << (64 * (m - m0))
        run = t >> 64
        hi_below = hi
    assert run in (0, 1)
    return limbs, run, allp


def phase0(K, c):
    c = sparse(c)
    return [stripe_value(K, c, s) for s in range(K.S)]


def carries(stripes):
    """carry into every stripe from the (generate, propagate) chain in product order"""
    cin, out = 0, []
    for _, g, p in stripes:
        out.append(cin)
        cin = g | (p & cin)
    return out


def phase1(K, stripes):
    """the stripes' final limbs (integers): carry-in added mod 2^(64 n)"""
    return [(x + ci) & ((1 << (64 * K.n(s))) - 1) for s, ((x, _, _), ci) in enumerate(zip(stripes, carries(stripes)))]


def assemble(K, limbs):
    return sum(x << (64 * K.ms[s]) for s, x in enumerate(limbs))


def product(K, c):
    """sum_k c_k 2^(k bits1) mod 2^(64 total), pairwise so that the shifts stay short"""
    c = sparse(c)
    if not c:
        return 0
    terms = [(k * K.bits1, v) for k, v in sorted(c.items())]   # (shift, value)
    while len(terms) > 1:
        nxt = [(terms[i][0], terms[i][1] + (terms[i + 1][1] << (terms[i + 1][0] - terms[i][0])))
               for i in range(0, len(terms) - 1, 2)]
        if len(terms) & 1:
            nxt.append(terms[-1])
        terms = nxt
    return (terms[0][1] << terms[0][0]) & ((1 << (64 * K.total)) - 1)


def _lead_ones(x, n):
    """leading (lowest) all-ones limbs of an n-limb value"""
    return min(n, (((x + 1) & ~x).bit_length() - 1) // 64)


def info(K, c):
    """per stripe: dict n, rank, g, p, cin, lead (all-ones limbs from the stripe's first limb on
    after phase 0: the limbs a carry-in of 1 wraps to zero)"""
    st = phase0(K, c)
    return [dict(s=s, n=K.n(s), rank=K.rank(s), g=g, p=p, cin=ci, lead=_lead_ones(x, K.n(s)))
            for s, ((x, g, p), ci) in enumerate(zip(st, carries(st)))]


# ---------------------------------------------------------------------------
# coefficient patterns (o = 2^bits1 - 1)
# ---------------------------------------------------------------------------
STOP_OFFSETS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)   # and n_s - 1


def ripple(K):
    """c_0 = o + 1, the rest o: the sum is 2^(len bits1), one carry from bit bits1 through every
    limb, stripe and rank up to there"""
    o = (1 << K.bits1) - 1
    c = {k: o for k in range(K.len)}
    c[0] = o + 1
    return c


def stop_bit(K, M):
    """(k, b): the lowest bit of limb M that lies in a coefficient k >= 1 of the ripple (bit b of
    c_k), or None where limb M has none (below bit bits1, or past the last coefficient)"""
    B = max(64 * M, K.bits1)
    k = B // K.bits1
    if B >= 64 * (M + 1) or k >= K.len:
        return None
    return k, B - k * K.bits1


def stop_limbs(K, stripes):
    """the product limbs of the `stop` cases: ms[s] + off for s in stripes and off in STOP_OFFSETS
    and n_s - 1, off < n_s, where the ripple reaches: [(s, off, M)]"""
    out = []
    for s in stripes:
        n = K.n(s)
        for off in sorted(set(STOP_OFFSETS) | {n - 1}):
            if 0 <= off < n and stop_bit(K, K.ms[s] + off) is not None:
                out.append((s, off, K.ms[s] + off))
    return out


def stop_stripes(K):
    """the first non-empty stripe after 0, the middle one and the last (a lone stripe: itself)"""
    ne = [s for s in range(K.S) if K.n(s)]
    return sorted({ne[min(1, len(ne) - 1)], ne[len(ne) // 2], ne[-1]})


def stop(K, M):
    """the ripple with the bit of stop_bit(M) cleared: the carry ends in limb M"""
    k, b = stop_bit(K, M)
    c = ripple(K)
    c[k] &= ~(1 << b)
    return c


def two_ripples(K):
    """a ripple from coefficient 0, stopped in the third non-empty stripe (with fewer than six: the
    second), and a second o + 1 at the first coefficient of the middle stripe (its own digit zero,
    its carry into the digits above): generate, propagate and kill all meet in the stripes'
    composition"""
    ne = [s for s in range(K.S) if K.n(s)]
    s1, smid = ne[2 if len(ne) >= 6 else min(1, len(ne) - 1)], ne[len(ne) // 2]
    M = K.ms[s1] + min(1, K.n(s1) - 1)
    c = stop(K, M) if stop_bit(K, M) is not None else ripple(K)
    k2 = smid * K.C if K.S > 1 else K.len // 2
    k2 = max(k2, stop_bit(K, M)[0] + 1 if stop_bit(K, M) is not None else 1)
    if k2 < K.len - 1:
        c[k2] = 1 << K.bits1
    return c


def halo_cases(K):
    """a single c_k = 2^N - 1 at k = s C - j, j = 1 .. H, for one s per rank (the rank's middle
    stripe that has coefficients), then at k = len - 1 alone: [(name, c)]"""
    top = (1 << K.N) - 1
    out, seen = [], set()
    for g in range(K.world):
        mine = [s for s in range(g, K.S, K.world) if 0 < s and s * K.C - 1 < K.len]
        if not mine:
            continue
        s = mine[len(mine) // 2]
        for j in range(1, K.H + 1):
            k = s * K.C - j
            if 0 <= k < K.len and k not in seen:
                seen.add(k)
                out.append((f"halo s{s}-{j}", {k: top}))
    out.append(("halo last", {K.len - 1: top}))
    return out


def cases(K, seed, stripes=None, halo=True):
    """every pattern of the placed combine tests: [(name, {k: c_k})].  stripes: the `stop` stripes
    (default stop_stripes)"""
    rng = random.Random(seed)
    out = [("ripple", ripple(K))]
    for s, off, M in stop_limbs(K, stop_stripes(K) if stripes is None else stripes):
        out.append((f"stop s{s}+{off}", stop(K, M)))
    out.append(("max", {k: (1 << K.N) - 1 for k in range(K.len)}))
    if halo:
        out += halo_cases(K)
    else:
        out.append(("halo last", {K.len - 1: (1 << K.N) - 1}))
    out.append(("two ripples", two_ripples(K)))
    out.append(("random", {k: rng.getrandbits(K.N) for k in range(K.len)}))
    out.append(("zero", {}))
    for _, c in out:
        check_range(K, c)
    return out


# the shapes of the placed shard combine test: (depth, w, n1, n2), the worlds, l, the k_combine1 form
SHAPES = [
    ((6, 1, 7, 6), (1, 2, 4), 1, "limb KM0"),
    ((8, 1, 100, 90), (1, 2, 4, 8), 4, "limb KM3"),
    ((11, 8, 20000, 20000), (1, 2, 4, 8), 256, "limb KM3"),
    ((8, 256, 40000, 40000), (1, 2, 4, 8), 1024, "consecutive KM4"),
    ((8, 512, 40000, 40000), (1, 2, 4), 2048, "consecutive KM3"),
    ((6, 4096, 100000, 100000), (1, 2, 8), 4096, "consecutive KM3"),
    # more than 256 stripes: k_stripe_carry's threads each compose a run of several stripes
    ((10, 1, 5000, 5000), (8,), 16, "limb KM3"),
]
SHAPE_WORLDS = [(sh, wd) for sh, worlds, _, _ in SHAPES for wd in worlds]
WHOLE_PATH = ((8, 256, 40000, 40000), 4)   # the one whole multiply (carry_operands) and its world


def check_shape_facts(K, shape, world):
    """what the (shape, world) entries of SHAPES are there for, asserted on the planner's Contract"""
    l, form = next((l, f) for s, _, l, f in SHAPES if s == shape)
    assert K.l == l and combine_form(K.N, K.bits1) == form, (shape, world)
    ns = [K.n(s) for s in range(K.S)]
    blocks = max(blocks_per_stripe(form, n) for n in ns)   # blocks holding limbs of a stripe
    facts = {
        ((6, 1, 7, 6), 2): K.H == 8 and K.C == 4,                        # the halo spans stripes and ranks
        ((6, 1, 7, 6), 4): K.H == 8 and K.C == 2 and ns.count(0) == 3,   # and three empty stripes
        ((8, 1, 100, 90), 8): K.H == 5 and K.C == 2 and 0 in ns,
        ((11, 8, 20000, 20000), 1): blocks == 2,
        ((11, 8, 20000, 20000), 8): K.Tr % 8 != 0,                       # uneven rows
        ((8, 256, 40000, 40000), 1): blocks == 2,
        ((8, 512, 40000, 40000), 1): blocks == 4,
        ((6, 4096, 100000, 100000), 1): blocks == 8,
        ((6, 4096, 100000, 100000), 2): blocks == 4,
        ((6, 4096, 100000, 100000), 8): K.C == 2 and K.C < K.H,
        ((10, 1, 5000, 5000), 8): K.S > 256,
    }
    assert facts.get((shape, world), True), (shape, world)


def combine_form(N, bits1):
    """the k_combine1 form exec.hpp's combine1 launches (comb_ct / comb_kw and its k3), restated"""
    kw = (N + 32767) // bits1 + 1
    if kw <= 4:
        return f"consecutive KM{3 if kw <= 3 else 4}"
    return "limb KM3" if (N + 63 + bits1 - 1) // bits1 <= 3 else "limb KM0"


def blocks_per_stripe(form, limbs):
    """k_combine1's blocks for a stripe of `limbs` limbs: 8 limbs per thread, 512 threads in the
    consecutive form and 256 in the per-limb form"""
    bl = 8 * (512 if form.startswith("consecutive") else 256)
    return (limbs + bl - 1) // bl


def carry_operands(K):
    """(a, b) whose product's coefficients are a ripple: a = 1 + sum over odd k of o 2^(k bits1),
    b = 1 + 2^bits1, so c = a * b digit-wise is (1, o + 1, o, o, ..., o, 0 ..): one carry from
    digit 1 through a run of all-ones limbs as long as a.  a, b < 2^(64 n) for n-limb operands of a
    balanced product."""
    o, n = (1 << K.bits1) - 1, K.total // 2
    a = 1 + sum(o << (k * K.bits1) for k in range(1, (64 * n) // K.bits1, 2))
    b = 1 + (1 << K.bits1)
    assert a < (1 << (64 * n))
    return a, b


def convolution(K, a, b):
    """{k: c_k} of the bits1-bit digits of a and b"""
    mask = (1 << K.bits1) - 1
    da = [(a >> (i * K.bits1)) & mask for i in range((a.bit_length() + K.bits1 - 1) // K.bits1)]
    db = [(b >> (i * K.bits1)) & mask for i in range((b.bit_length() + K.bits1 - 1) // K.bits1)]
    c = {}
    for i, x in enumerate(da):
        for j, y in enumerate(db):
            if x and y:
                c[i + j] = c.get(i + j, 0) + x * y
    return c
