// nega.hpp -- the negacyclic top level: products mod M = 2^B + 1 (B = 64 L) as a length-2n
// negacyclic convolution of bits1-bit pieces, B = 2n bits1 (the reference's fft_mulmod_2expp1,
// mul_fft.c:2998-3167).  Between the kernels here run the multiply's untruncated
// stages (Exec): forward columns and rows, pointwise, inverse rows and columns.
//   k_nweight<U>     piece j of the operand (fused split; the top limb enters piece 0 as -a[L]:
//                    2^B == -1) times theta^j, theta = sqrt2^w the 4n-th root of unity, reduced store
//   k_nunweight<U>   slot j times theta^-j 2^-(depth+1), canonical store (the register-pass plans
//                    with even w take k_rscale's per-slot exponent instead)
//   k_nwrap<V>       the scratch sum T = sum c~_j 2^(j bits1) of the canonical coefficients
//                    (k_combine1) folded mod M with the signs read back: a decoupled look-back
//                    carry chain over the L result limbs (nega_chain, shared with negaw.hpp)
//   k_nfix           the end-around correction: minus the chain's overflow (2^B == -1)
#pragma once
#include "kernels.hpp"
#include "combine.hpp"

struct NegaArgs {
    u64 *dig[2];
    u64 *cb[2];
    int *top[2];
    const u64 *src[2];   // k_nweight: the operands, L + 1 limbs each
    long L;
    u64 bits1, N, w;
    int l, depth;
    unsigned *zp;        // k_nweight: clear zp[0, zn) (the combine's look-back flags)
    long zn;
};

// the launch's threads clear NegaArgs::zp, before any barrier (as pass_clear_flags)
__device__ inline void nega_clear_flags(const NegaArgs &a)
{
    if (!a.zp) return;
    const long nt = blockDim.x, nthr = (long)gridDim.x * gridDim.y * nt;
    const long t = ((long)blockIdx.y * gridDim.x + blockIdx.x) * nt + threadIdx.x;
    for (long i = t; i < a.zn; i += nthr) a.zp[i] = 0u;
}

// threads per workgroup at most (Exec::nega_tpb): l <= 256 one limb per thread, l <= 1024 two over
// <= 512 threads, l = 2048 and 4096 four (two over 1024 threads would spill)
#define NEGA_LB(U) ((U) == 1 ? 256 : (U) == 2 ? 512 : 1024)

// one workgroup per slot j (blockIdx.x) and operand (blockIdx.y)
template <int U>
__global__ __launch_bounds__(NEGA_LB(U)) void k_nweight(NegaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    nega_clear_flags(a);
    const WG c = wg_ctx();
    const int l = a.l;
    constexpr int RB = s2_rb(U);
    const Lds sm = lds_carve<U, 3>(smem, l, RB, c.nw);
    const int op = blockIdx.y;
    Coef st;
    st.dig = a.dig[op];
    st.cb = a.cb[op];
    st.top = a.top[op];
    const long j = blockIdx.x;
    long slot[3] = {j, j, j};
    bool keep[3] = {false, true, false};
    i64 x[3][2 * U];
    zero_coeff<U>(x[0]);
    zero_coeff<U>(x[2]);
    const SrcSlice whole{0, 1, 0};
    load_split<U>(c, x[1], a.src[op], a.L, whole, j, a.bits1, l);
    if (j == 0 && c.t == 0) x[1][0] -= (i64)a.src[op][a.L];   // 0 or 1: 2^B == -1
    s2_root<U>(c, x, (u64)j, a.w, a.N, l, sm.stage, RB);
    normalize_store<U, 3>(c, x, slot, keep, false, st, l, sm);
}

// slot j <- theta^(4n - j) 2^(2N - (depth + 1)) slot j, canonical
template <int U>
__global__ __launch_bounds__(NEGA_LB(U)) void k_nunweight(NegaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int l = a.l;
    constexpr int RB = s2_rb(U);
    const Lds sm = lds_carve<U, 3>(smem, l, RB, c.nw);
    Coef st;
    st.dig = a.dig[0];
    st.cb = a.cb[0];
    st.top = a.top[0];
    const long j = blockIdx.x;
    long slot[3] = {j, j, j};
    bool keep[3] = {false, true, false};
    i64 x[3][2 * U];
    zero_coeff<U>(x[0]);
    zero_coeff<U>(x[2]);
    load_coeff<U>(c, x[1], st, j, l);
    s2_root<U>(c, x, ((u64)4 << a.depth) - (u64)j, a.w, a.N, l, sm.stage, RB, 2 * a.N - (u64)(a.depth + 1));
    normalize_store<U, 3>(c, x, slot, keep, true, st, l, sm);
}

// --------------------------------------------------------------------------
// The fold.  With s_j = 1 where c~_j > p/2 (the signed coefficient is c~_j - p, p = 2^N + 1),
//   r == T - sum_j s_j (2^N + 1) 2^(j bits1)   (mod M),   T = sum_j c~_j 2^(j bits1).
// k_combine1 reads a coefficient's limbs only, so the canonical 2^N (top = 1, limbs 0: c = -1)
// is missing from T: for those j the 2^N terms cancel and only -2^(j bits1) is left.
// Every term is cut into B-bit pieces, piece i weighing (-1)^i (2^B == -1):
//   T_i       limbs [i L, (i + 1) L) of T                           sign (-1)^i
//   Sa        bits j bits1, s_j = 1                                  sign -
//   Sb_q      bits j bits1 + N - q B in [0, B), s_j = 1, top_j = 0   sign -(-1)^q
// A negative piece X < 2^B enters as its B-bit complement: -X == ~X + 2 (mod M).  The pieces'
// limbs are summed per result limb (64 bits + a small overflow into the next limb), which
// leaves a sum of two numbers: a binary carry chain, resolved as in k_combine1 (ticketed
// blocks, flags 0 not ready / 2 propagate / 4, 5 carry-out).  What leaves limb L - 1 -- the
// last limb's overflow plus the chain's carry-out, O -- weighs 2^B == -1: k_nfix subtracts it.
// --------------------------------------------------------------------------
struct NegaCombArgs {
    const u64 *T;        // the scratch sum, TL limbs
    long TL;
    const u64 *dig;      // canonical coefficients (slot j = coefficient j)
    const int *top;
    int l;
    u64 N, bits1;
    long L;              // result limbs below the top limb
    long len;            // 2n coefficients
    int nT;              // pieces of T: ceil(TL / L)
    int qmax;            // last piece index of the bits j bits1 + N
    u32 K;               // 2 x the negative pieces
    double inv_bits1;
    long nblk;           // blocks; st[nblk]: the ticket counter, st[nblk + 1]: O
};

// sign of coefficient j: its canonical value is above p/2 (bit N - 1, or the carry limb)
__device__ __forceinline__ bool nega_neg(const NegaCombArgs &a, long j, bool *is2N)
{
    const int tp = a.top[j];
    *is2N = tp != 0;
    return tp != 0 || (a.dig[(size_t)j * a.l + a.l - 1] >> 63) != 0;
}

// the pieces' sum at result limb m: 64 bits and the overflow into limb m + 1
__device__ __forceinline__ void nega_limb(const NegaCombArgs &a, long m, u64 *lo, u32 *hi)
{
    u64 slo = 0;
    u32 shi = 0;
    auto add = [&](u64 v) {
        u64 t;
        shi += add_ovf(slo, v, &t);
        slo = t;
    };
    for (int i = 0; i < a.nT; ++i) {
        const long q = (long)i * a.L + m;
        const u64 v = q < a.TL ? a.T[q] : 0;
        add(i & 1 ? ~v : v);
    }
    const i64 P = (i64)m * 64, B = (i64)a.L * 64;
    // bit j bits1 - X for the negative coefficients j with j bits1 in [X, X + 64) (X may be below 0)
    auto bits = [&](i64 X, bool skip2N) {
        u64 v = 0;
        long j = X > 0 ? udiv_inv((u64)(X - 1), a.bits1, a.inv_bits1) + 1 : 0;   // ceil(X / bits1)
        for (; j < a.len; ++j) {
            const i64 pos = (i64)((u64)j * a.bits1);
            if (pos >= X + 64) break;
            bool t2;
            if (nega_neg(a, j, &t2) && !(skip2N && t2)) v |= (u64)1 << (pos - X);
        }
        return v;
    };
    add(~bits(P, false));
    for (int q = 0; q <= a.qmax; ++q) {   // j bits1 + N - q B in [P, P + 64)
        const u64 v = bits(P + (i64)q * B - (i64)a.N, true);
        add(q & 1 ? v : ~v);
    }
    if (m == 0) add((u64)a.K);
    *lo = slo;
    *hi = shi;
}

// The chain over the L result limbs, shared by k_nwrap and k_nwrapw (negaw.hpp): limb(m, &lo, &hi)
// gives the pieces' sum at result limb m; nblk blocks of 256 threads, V limbs per thread.
template <int V, class LimbFn>
__device__ __forceinline__ void nega_chain(long L, long nblk, LimbFn limb, u64 *r, u32 *st)
{
    constexpr int NT = 256, BL = NT * V;
    __shared__ u32 H[NT + 1];
    __shared__ u64 scr[64];
    __shared__ u32 sh_cin, sh_b, sh_htop;
    const WG c = wg_ctx();
    if (c.t == 0) sh_b = __hip_atomic_fetch_add(&st[nblk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const long b = sh_b;   // ticket: every block below it has started
    const long base = b * BL, mA = base + (long)c.t * V;
    u64 lo[V], v[V];
    u32 hi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        lo[k] = 0;
        hi[k] = 0;
        if (mA + k < L) limb(mA + k, &lo[k], &hi[k]);
        if (mA + k == L - 1) sh_htop = hi[k];
    }
    H[c.t + 1] = hi[V - 1];
    if (c.t == 0) {
        u64 l0 = 0;
        u32 h0 = 0;
        if (base > 0) limb(base - 1, &l0, &h0);
        H[0] = h0;
    }
    __syncthreads();
    u32 g = 0, p = 0;
    bool G = false, Pa = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const bool real = mA + k < L;
        const bool gk = add_ovf(lo[k], (u64)(k ? hi[k - 1] : H[c.t]), &v[k]) && real;
        const bool pk = v[k] == MPF_MAXL || !real;
        g |= (u32)gk << k;
        p |= (u32)pk << k;
        G = gk || (pk && G);
        Pa = Pa && pk;
    }
    u32 co0;
    wg_scan<1>(c, G, Pa, 0, &co0, scr);
    const bool allp = __syncthreads_and(Pa);
    if (c.t == 0) {   // look-back
        u32 cin = 0;
        if (b == 0) {
            __hip_atomic_store(&st[0], 4u + co0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const u32 agg = co0 ? 1u : (allp ? 2u : 3u);
            __hip_atomic_store(&st[b], agg == 1u ? 5u : agg == 2u ? 2u : 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (long q = b - 1;; --q) {
                u32 f;
                while ((f = __hip_atomic_load(&st[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
                    __builtin_amdgcn_s_sleep(1);
                if (f >= 4u) { cin = f - 4u; break; }
            }
            if (agg == 2u) __hip_atomic_store(&st[b], 4u + cin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        sh_cin = cin;
    }
    __syncthreads();
    u32 co;
    const u32 ci = wg_scan<1>(c, G, Pa, sh_cin, &co, scr);
    bool run = ci & 1;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (mA + k < L) r[mA + k] = v[k] + (run ? 1 : 0);
        run = ((g >> k) & 1) || (((p >> k) & 1) && run);
    }
    if (c.t == 0 && b == nblk - 1) st[nblk + 1] = sh_htop + co;   // what leaves limb L - 1
}

template <int V>
__global__ __launch_bounds__(256) void k_nwrap(NegaCombArgs a, u64 *r, u32 *st)
{
    nega_chain<V>(a.L, a.nblk, [&](long m, u64 *lo, u32 *hi) { nega_limb(a, m, lo, hi); }, r, st);
}

// r (L limbs, V < 2^B) <- V - O mod M, fully reduced, and the top limb r[L].  One workgroup: the
// borrow passes the zero limbs above limb 0 only (as k_stripe_carry's all-ones limbs, almost
// never past the first); when every limb is zero, V < O and the result is M - (O - V).
__global__ __launch_bounds__(1024) void k_nfix(u64 *r, long L, const u32 *st, long nblk)
{
    __shared__ unsigned long long first, sv0;
    const int t = threadIdx.x;
    if (t == 0) {
        sv0 = r[0];
        first = (unsigned long long)L;   // the first non-zero limb above limb 0 (L: none)
    }
    __syncthreads();   // every thread has limb 0's value before anything is written
    const u64 O = st[nblk + 1], v0 = sv0;
    if (v0 >= O) {
        if (t == 0) {
            r[0] = v0 - O;
            r[L] = 0;
        }
        return;
    }
    for (long c0 = 1; c0 < L; c0 += 1024) {
        const long m = c0 + t;
        const u64 nz = __ballot(m < L && r[m] != 0);
        if ((t & 63) == 0 && nz) atomicMin(&first, (unsigned long long)(m + __builtin_ctzll(nz)));
        __syncthreads();
        const bool found = first < (unsigned long long)L;
        __syncthreads();   // read by all before the next chunk's atomicMin
        if (found) break;
    }
    const long f = (long)first;
    const u64 d = O - v0;   // >= 1
    if (f == L && d == 1) {   // M - 1 = 2^B: limbs 1 .. L - 1 are zero already
        if (t == 0) {
            r[0] = 0;
            r[L] = 1;
        }
        return;
    }
    for (long m = 1 + t; m < f; m += 1024) r[m] = MPF_MAXL;
    if (t == 0) {
        if (f < L) {
            r[f] -= 1;
            r[0] = v0 - O;             // mod 2^64
        } else {
            r[0] = MPF_MAXL - (d - 2);   // M - d = (2^B - 1) - (d - 2)
        }
        r[L] = 0;
    }
}
