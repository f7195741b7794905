"""Placed-coefficient tests of the combine (csrc/combine.hpp): k_combine1 in its four production
forms, k_comb_summary and k_stripe_carry through mpfft_shard_combine with every rank on device 0,
and the single stripe of MPFFT_STAGE_COMBINE, against the exact stripe model of
tests/combine_model.py.

Random products never carry between stripes (a stripe's carry-out needs a window sum to overflow
its limb: about 2^-64 per boundary), so the canonical coefficients are placed by hand here:
`ripple` (one carry through every limb, stripe and rank), `stop` (the ripple ended at the chunk
edges of k_stripe_carry and the block edges of k_combine1), `max` (every window sum's overflow at its
largest, handed across every stripe boundary), single coefficients at every halo distance, two
ripples with a stop between them, random and zero (combine_model.cases).  Everything the kernels
may not read or write is poisoned: coefficient slots from len on, halo slots of coefficients below
0, the stripe buffers, the scratch and the summaries, with guard regions around each array.  After
phase 0 every stripe's limbs and its (generate, propagate) summary must be the model's; after phase
1 the assembled stripes must be sum c_k 2^(k bits1) mod 2^(64 total), and the limbs of a stripe
buffer past the stripe's end must still hold the poison.
"""
import numpy as np
import pytest

import combine_model as cm
import stage_model as sm
from helpers import to_int
from test_gpu_stage_adversarial import Bench

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A5A5A5A5A
ROWS = pytest.mark.parametrize("row", sm.TABLE, ids=[r["id"] for r in sm.TABLE])
SW = pytest.mark.parametrize("shape,world", cm.SHAPE_WORLDS, ids=[f"{s[0]}-{s[1]}-{s[2]}-w{w}" for s, w in cm.SHAPE_WORLDS])


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def natural(K, c, slots, l):
    """the coefficients in natural order as (slots, l) limbs: c_k for k < len, poison from len on"""
    nat = np.full((slots, l), POISON, np.uint64)
    nat[:K.len] = 0
    for k, v in c.items():
        nat[k] = np.frombuffer(v.to_bytes(8 * l, "little"), dtype=np.uint64)
    return nat


def limbs_of(x, n):
    return np.frombuffer(x.to_bytes(8 * n, "little"), dtype=np.uint64)


class Guarded:
    """a device array between two poisoned guard regions (a read outside the array sees poison, a
    write outside it is found)"""

    def __init__(self, torch, dev, count, guard, dtype=None):
        self.torch, self.n, self.g = torch, count, guard
        self.dtype = dtype or torch.int64
        self.all = torch.empty(count + 2 * guard, dtype=self.dtype, device=dev)
        self.fill = {torch.int64: POISON, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}[self.dtype]
        self.all.fill_(self.fill)
        self.view = self.all[guard: guard + count]

    def poison(self):
        self.view.fill_(self.fill)

    def put(self, arr):
        self.view.copy_(self.torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.int64)))

    def get(self):
        a = self.view.cpu().numpy()
        return a.view(np.uint64) if self.dtype == self.torch.int64 else a

    def guards_intact(self):
        g = self.g
        return bool((self.all[:g] == self.fill).all() and (self.all[g + self.n:] == self.fill).all())


class ShardRig:
    """every rank's combine arrays of one (shape, world) on one device"""

    def __init__(self, mp, dev, shape, world):
        import torch
        depth, w, n1, n2 = shape
        self.mp, self.torch, self.world = mp, torch, world
        self.K = K = cm.shard_contract(mp, n1, n2, depth, w, world)   # a rejected world raises: a failure
        part = mp.shard_partition(n1, n2, depth, w, world)
        self.part = part
        guard = K.l * (K.H + 2) + 64
        self.col = [Guarded(torch, dev, K.Tr * K.C * K.l, guard) for _ in range(world)]
        self.halo = [Guarded(torch, dev, K.Tr * K.H * K.l, guard) for _ in range(world)]
        self.out = [Guarded(torch, dev, K.Tr * K.SL, 64) for _ in range(world)]
        self.sums = [Guarded(torch, dev, 2 * K.Tr, 16, torch.int32) for _ in range(world)]
        nb = mp.shard_combine_tmp_bytes(n1, n2, depth, w, world)
        assert nb > 0
        self.tmp = [Guarded(torch, dev, nb, 256, torch.uint8) for _ in range(world)]
        # the combine reads the column layout's limbs only: the other arrays of the descriptor are
        # small dummies
        dummy = {"dig": torch.zeros(8, dtype=torch.int64, device=dev), "cb": torch.zeros(8, dtype=torch.int64, device=dev),
                 "top": torch.zeros(8, dtype=torch.int32, device=dev)}
        self.desc = []
        for g in range(world):
            colg = dict(dummy, dig=self.col[g].view)
            self.desc.append(mp.shard_desc(dict(n1=n1, n2=n2, depth=depth, w=w, c0=g * K.C, ccount=K.C, r0=part["rows"][g],
                                                rcount=part["rows"][g + 1] - part["rows"][g], ccb=K.C,
                                                col=[colg, colg], row=[dummy, dummy])))
        self._keep = dummy

    def place(self, c):
        K, W = self.K, self.world
        nat = natural(K, c, K.Tr * K.NC, K.l)
        pad = np.concatenate([np.full((K.H, K.l), POISON, np.uint64), nat,
                              np.full((K.H, K.l), POISON, np.uint64)])   # pad[k + H] = c_k
        for g in range(W):
            self.col[g].put(nat.reshape(K.Tr, W, K.C, K.l)[:, g])
            # stripe j's halo: coefficients s C - H .. s C - 1, s = j W + g, filled from the list
            idx = (np.arange(K.Tr)[:, None] * W + g) * K.C + np.arange(K.H)[None, :]
            self.halo[g].put(pad[idx])
            for a in (self.out[g], self.sums[g], self.tmp[g]):
                a.poison()

    def phase(self, ph, sums_all=None):
        for g in range(self.world):
            self.mp.shard_combine(self.desc[g], ph, self.out[g].view, self.halo[g].view, self.sums[g].view, sums_all,
                                  self.tmp[g].view)
        self.torch.cuda.synchronize()

    def expected(self, limbs):
        """the ranks' stripe buffers holding the stripes' limbs (integers), poison elsewhere"""
        K, W = self.K, self.world
        want = [np.full(K.Tr * K.SL, POISON, np.uint64) for _ in range(W)]
        for s, x in enumerate(limbs):
            g, j, n = s % W, s // W, K.n(s)
            want[g][j * K.SL: j * K.SL + n] = limbs_of(x, n)
        return want

    def first_diff(self, got, want):
        """(stripe, limb) of the first differing limb of the ranks' stripe buffers, or None"""
        K, W = self.K, self.world
        for g in range(W):
            bad = np.nonzero(got[g] != want[g])[0]
            if len(bad):
                j, m = divmod(int(bad[0]), K.SL)
                return j * W + g, m
        return None

    def run(self, name, c, fails):
        K, W = self.K, self.world
        tag = f"{name} (world {W})"
        self.place(c)
        st = cm.phase0(K, c)
        self.phase(0)
        got = [o.get() for o in self.out]
        d = self.first_diff(got, self.expected([x for x, _, _ in st]))
        if d:
            fails.append(f"{tag}: phase 0 stripe {d[0]} (rank {d[0] % W}, {K.n(d[0])} limbs) differs at limb {d[1]}")
        sums = [s.get() for s in self.sums]
        for s, (_, gen, prop) in enumerate(st):
            g, j = s % W, s // W
            if (int(sums[g][2 * j]), int(sums[g][2 * j + 1])) != (gen, prop):
                fails.append(f"{tag}: stripe {s} (rank {g}) summary {tuple(int(v) for v in sums[g][2 * j: 2 * j + 2])} "
                             f"want {(gen, prop)}")
                break
        # every rank's summaries in rank order, as an all-gather leaves them
        self.phase(1, self.torch.cat([s.view for s in self.sums]))
        got = [o.get() for o in self.out]
        final = cm.phase1(K, st)
        d = self.first_diff(got, self.expected(final))
        if d:
            what = "past the stripe's end" if d[1] >= K.n(d[0]) else f"carry-in {cm.carries(st)[d[0]]}"
            fails.append(f"{tag}: phase 1 stripe {d[0]} (rank {d[0] % W}, {K.n(d[0])} limbs) differs at limb {d[1]} ({what})")
        prod = to_int(self.mp.assemble_stripes(self.part, W, got))
        if prod != cm.product(K, c):
            fails.append(f"{tag}: the assembled stripes are not sum c_k 2^(k bits1)")
        for kind, arrs in (("coefficients", self.col), ("halo", self.halo), ("stripes", self.out), ("summaries", self.sums),
                           ("scratch", self.tmp)):
            if not all(a.guards_intact() for a in arrs):
                fails.append(f"{tag}: wrote outside the {kind} array")


@SW
def test_shard_combine_placed(mp, torch_dev, shape, world):
    """mpfft_shard_combine phases 0 and 1 on every rank of the (shape, world) table, every pattern"""
    R = ShardRig(mp, torch_dev, shape, world)
    K = R.K
    cm.check_shape_facts(K, shape, world)
    fails = []
    for name, c in cm.cases(K, 100 + world):
        R.run(name, c, fails)
        if len(fails) > 6:
            break
    assert not fails, "\n".join(fails)


@ROWS
def test_single_combine_placed(mp, torch_dev, row):
    """MPFFT_STAGE_COMBINE (combine_single: one stripe, k_combine1 on fold plans too) on the
    coefficients placed canonically in operand A's slots; the stop offsets from limb 0 of the
    product.  The stage clears its look-back flags itself (only the whole multiply has the first
    forward pass clear them), so the whole workspace starts as 0x5A."""
    import torch
    B = Bench(mp, torch_dev, row)
    S = B.S
    total = B.n1 + B.n2
    K = cm.single_contract(S.N, S.bits1, S.j1 + S.j2 - 1, total)
    lay, l = B.lay, S.l
    dr = Guarded(torch, torch_dev, total, 64)
    B.dr = dr.view
    u8 = B.ws.view(torch.uint8)
    fails = []
    for name, c in cm.cases(K, 200 + l, stripes=[0], halo=False):
        B.poison()
        dr.poison()
        nat = natural(K, c, K.len, l)
        u8[lay["digA"]: lay["digA"] + K.len * l * 8].copy_(torch.from_numpy(nat.reshape(-1).view(np.uint8)))
        u8[lay["topA"]: lay["topA"] + K.len * 4].zero_()
        u8[lay["cbA"]: lay["cbA"] + K.len * lay["cbw"] * 8].zero_()
        B.stage(mp.STAGE_COMBINE)
        torch.cuda.synchronize()
        got, want = to_int(dr.get()), cm.product(K, c)
        if got != want:
            x = got ^ want
            fails.append(f"{name} [{row['id']}]: lowest wrong limb {((x & -x).bit_length() - 1) // 64} of {total}")
        if not dr.guards_intact():
            fails.append(f"{name} [{row['id']}]: wrote past the product")
        if len(fails) > 6:
            break
    assert not fails, "\n".join(fails)


def test_mul_multi_carry_through_ranks(mp, torch_dev):
    """one whole multiply (mpfft_mul_multi_device, four ranks on device 0) whose coefficients are a
    ripple (combine_model.carry_operands; its stripes checked on the CPU in test_combine_model.py):
    k_stripe_carry's add path wraps all-ones stripes of several ranks inside a real product"""
    import torch
    (depth, w, n1, n2), world = cm.WHOLE_PATH
    K = cm.shard_contract(mp, n1, n2, depth, w, world)
    ai, bi = cm.carry_operands(K)
    a, b = limbs_of(ai, n1).copy(), limbs_of(bi, n2).copy()
    part = mp.shard_partition(n1, n2, depth, w, world)
    src1 = [torch.from_numpy(mp.shard_pack(a, n1, n2, depth, w, world, g).view(np.int64)).to(torch_dev) for g in range(world)]
    src2 = [torch.from_numpy(mp.shard_pack(b, n1, n2, depth, w, world, g).view(np.int64)).to(torch_dev) for g in range(world)]
    outs = [torch.full((part["Tr"] * part["SL"],), -1, dtype=torch.int64, device=torch_dev) for _ in range(world)]
    try:
        mp.mul_multi_device(n1, n2, depth, w, [0] * world, src1, src2, outs)
        got = to_int(mp.assemble_stripes(part, world, [o.cpu().numpy().view(np.uint64) for o in outs]))
    finally:
        mp.multi_release()
    assert got == ai * bi
