// cyc.hpp -- the cyclic top level: products mod M = 2^B - 1 (B = 64 L) as a length-2n cyclic
// convolution of bits1-bit pieces, B = 2n bits1.  The untruncated transform computes
// that convolution as it stands, so the multiply's stages (Exec) run unchanged -- the first column
// pass splits the operands, no weight, the plain scaling -- and only the fold is new:
//   k_cwrap<V>   the scratch sum T = sum c_j 2^(j bits1) of the canonical coefficients (k_combine1)
//                cut into B-bit pieces, every one of sign + (2^B == 1), summed per result limb: a
//                decoupled look-back carry chain over the L result limbs
//   k_cfix       the end-around carry: plus what left limb L - 1, and all-ones (== 0) stored as 0
#pragma once
#include "kernels.hpp"
#include "combine.hpp"

struct CycCombArgs {
    const u64 *T;   // the scratch sum, TL limbs
    long TL;
    long L;         // result limbs
    int nT;         // pieces of T: ceil(TL / L)
    long nblk;      // blocks; st[nblk]: the ticket counter, st[nblk + 1]: O, st[nblk + 2 + b]: block b has a
                    // limb above limb 0 that is not all-ones (a word per block, each written once: no
                    // atomic on one address, nothing to clear)
};

// the pieces' sum at result limb m: 64 bits and the overflow into limb m + 1 (below nT)
__device__ __forceinline__ void cyc_limb(const CycCombArgs &a, long m, u64 *lo, u32 *hi)
{
    u64 slo = 0;
    u32 shi = 0;
    for (int i = 0; i < a.nT; ++i) {
        const long q = (long)i * a.L + m;
        if (q >= a.TL) break;
        u64 t;
        shi += add_ovf(slo, a.T[q], &t);
        slo = t;
    }
    *lo = slo;
    *hi = shi;
}

// With S_m = lo_m + 2^64 hi_m the sum is sum_m (lo_m + hi_(m-1)) 2^(64 m) + hi_(L-1) 2^B.  Adding
// hi_(m-1) generates a carry or not, and a limb that generated is below hi_(m-1), never all-ones:
// a binary carry chain, resolved as in k_combine1 and k_nwrap (ticketed blocks, lower blocks
// always started first; flags 0 not ready / 2 propagate / 4, 5 carry-out).  What leaves limb
// L - 1 -- the last limb's overflow plus the chain's carry-out, O <= nT -- weighs 2^B == 1:
// k_cfix adds it at limb 0.
template <int V>
__global__ __launch_bounds__(256) void k_cwrap(CycCombArgs a, u64 *r, u32 *st)
{
    constexpr int NT = 256, BL = NT * V;
    __shared__ u32 H[NT + 1];
    __shared__ u64 scr[64];
    __shared__ u32 sh_cin, sh_b, sh_htop;
    const WG c = wg_ctx();
    if (c.t == 0) sh_b = __hip_atomic_fetch_add(&st[a.nblk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const long b = sh_b;   // ticket: every block below it has started
    const long base = b * BL, mA = base + (long)c.t * V;
    u64 lo[V], v[V];
    u32 hi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        lo[k] = 0;
        hi[k] = 0;
        if (mA + k < a.L) cyc_limb(a, mA + k, &lo[k], &hi[k]);
        if (mA + k == a.L - 1) sh_htop = hi[k];
    }
    H[c.t + 1] = hi[V - 1];
    if (c.t == 0) {
        u64 l0 = 0;
        u32 h0 = 0;
        if (base > 0) cyc_limb(a, base - 1, &l0, &h0);
        H[0] = h0;
    }
    __syncthreads();
    u32 g = 0, p = 0;
    bool G = false, Pa = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const bool real = mA + k < a.L;
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
    bool run = ci & 1, low = false;   // low: a limb above limb 0 that is not all-ones
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (mA + k < a.L) {
            const u64 out = v[k] + (run ? 1 : 0);
            r[mA + k] = out;
            low = low || (mA + k > 0 && out != MPF_MAXL);
        }
        run = ((g >> k) & 1) || (((p >> k) & 1) && run);
    }
    const bool anylow = __syncthreads_or(low);
    if (c.t == 0) {
        st[a.nblk + 2 + b] = anylow ? 1u : 0u;
        if (b == a.nblk - 1) st[a.nblk + 1] = sh_htop + co;   // what leaves limb L - 1
    }
}

// r (L limbs, R < 2^B) <- R + O mod M, fully reduced (all-ones, == 0, is stored as 0).  One
// workgroup.  The carry out of limb 0 passes all-ones limbs only (almost never past the first); if
// it leaves limb L - 1 it comes round as one more 1 at limb 0, which by then holds less than O and
// cannot carry again.
__global__ __launch_bounds__(1024) void k_cfix(u64 *r, long L, const u32 *st, long nblk)
{
    __shared__ unsigned long long first;
    const int t = threadIdx.x;
    const u64 O = st[nblk + 1], v0 = r[0];
    bool low = false;
    for (long b = t; b < nblk; b += 1024) low = low || st[nblk + 2 + b] != 0;
    if (t == 0) first = (unsigned long long)L;   // the first limb above limb 0 that is not all-ones (L: none)
    // (the barrier: every thread has limb 0's value before anything is written)
    const bool ones_above = !__syncthreads_or(low);   // limbs 1 .. L - 1 are all all-ones (or L == 1)
    u64 s0;
    if (!add_ovf(v0, O, &s0)) {
        if (s0 == MPF_MAXL && ones_above) {   // M == 0
            for (long m = t; m < L; m += 1024) r[m] = 0;
        } else if (t == 0 && O) {
            r[0] = s0;
        }
        return;
    }
    // s0 < O from here on
    if (ones_above) {   // the carry leaves limb L - 1 and comes round
        for (long m = 1 + t; m < L; m += 1024) r[m] = 0;
        if (t == 0) r[0] = s0 + 1;
        return;
    }
    for (long c0 = 1; c0 < L; c0 += 1024) {
        const long m = c0 + t;
        const u64 nz = __ballot(m < L && r[m] != MPF_MAXL);
        if ((t & 63) == 0 && nz) atomicMin(&first, (unsigned long long)(m + __builtin_ctzll(nz)));
        __syncthreads();
        const bool found = first < (unsigned long long)L;
        __syncthreads();   // read by all before the next chunk's atomicMin
        if (found) break;
    }
    const long f = (long)first;   // < L: the flag said so
    for (long m = 1 + t; m < f; m += 1024) r[m] = 0;
    if (t == 0) {
        if (f < L) r[f] += 1;
        r[0] = s0;
    }
}
