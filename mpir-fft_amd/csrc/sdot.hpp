// sdot.hpp -- signed sums of products (mpfft_sdot_*): r = sum_pos a_i b_i - sum_neg a_i b_i on the
// dot plan, with unsigned transforms throughout.  X = 2^(64 n1).  A term that is subtracted feeds the
// transforms the limb-wise complement ~a_i = X - 1 - a_i (n1 limbs, non-negative, the same pieces
// count), so the sum run_dot forms is r' = r + (X - 1) D with D = sum_neg b_i (at most n2 + 1 limbs),
// and r = r' - X D + D mod 2^(64 (n1 + n2 + 1)): the two's-complement value.  Every piece stays in
// [0, 2^bits1) and every coefficient below 2^N under the dot plan's own bits1, so nothing of the
// transform, pointwise, inverse or combine code differs from the unsigned sum's.
//   k_sdneg   per negative term, in front of its forward columns: ~a_i into a scratch the split reads
//             in place of a_i, and D <- b_i (the first negative term) or D <- D + b_i.
//   k_sdedge, k_sdfix   once behind the combine: d_r <- d_r + D - (D << 64 n1), in place.
// D is kept in carry-save form: a limb array Dl and a byte per limb Dc counting the overflows of that
// limb's additions (at most 63 for 64 terms) -- D = sum_i (Dl[i] + 2^64 Dc[i]) 2^(64 i) -- so a term
// costs no carry chain; the one chain is k_sdfix's, and it is fold.hpp's (cf_chain_block).
// Included by mpfft.hip after fold.hpp.
#pragma once
#include "fold.hpp"

#define SDFIX_NT 512                 // threads per k_sdfix block, 8 limbs each (as k_combine_red)
#define SDFIX_CB (8 * SDFIX_NT)      // limbs per chain block (MPFFT_SDOT_FIX_BLOCK)

struct SdArgs {
    u64 *Dl;              // D's limbs, n2
    unsigned char *Dc;    // D's per-limb overflow counts, n2
    u32 *st;              // k_sdfix's look-back flags [0, nb) and ticket counter st[nb]
    int *edge;            // edge[b]: the overflow of limb b SDFIX_CB - 1 (the limb below block b), edge[0] = 0
    long n1, n2, total;   // total = n1 + n2 + 1
    long nb;              // chain blocks
};

// ---- k_sdneg: the pre-pass of one negative term ----------------------------------------------
// scr[i] = ~a[i] (i < n1); Dl[i], Dc[i] <- b[i], 0 (init) or the carry-save sum with b[i] (i < n2).
// a and b are only read and may be the same array; scr, Dl and Dc are only written here.  Four limbs
// per thread, 256 limbs apart (coalesced 8-byte accesses: the operands need not be 16-byte aligned).
__global__ __launch_bounds__(256) void k_sdneg(const u64 *a, const u64 *b, u64 *scr, SdArgs d, int init)
{
    const long i0 = (long)blockIdx.x * 1024 + threadIdx.x;
    u64 av[4], bv[4], dv[4];
    unsigned char cv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // every load requested before any is used
        const long i = i0 + 256 * k;
        av[k] = i < d.n1 ? a[i] : 0;
        bv[k] = i < d.n2 ? b[i] : 0;
        dv[k] = !init && i < d.n2 ? d.Dl[i] : 0;
        cv[k] = !init && i < d.n2 ? d.Dc[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + 256 * k;
        if (i < d.n1) scr[i] = ~av[k];
        if (i < d.n2) {
            const u64 t = dv[k] + bv[k];
            d.Dl[i] = t;
            d.Dc[i] = (unsigned char)(cv[k] + (t < bv[k] ? 1 : 0));
        }
    }
}

// ---- the correction ---------------------------------------------------------------------------
// Limb m of d_r + D - (D << 64 n1) before the chain, as a 128-bit signed sum (lo, hi), |hi| <= 2:
// rv + Dl[m] + Dc[m - 1] - Dl[m - n1] - Dc[m - n1 - 1], each where its index is in [0, n2).  (The top
// overflow count Dc[n2 - 1] lands at limb n2 and, subtracted, at limb n1 + n2 = total - 1.)
__device__ __forceinline__ void sd_limb(const SdArgs &d, long m, u64 rv, u64 *plo, int *phi)
{
    const long j = m - d.n1;
    const u64 p0 = m < d.n2 ? d.Dl[m] : 0;
    const u64 p1 = m >= 1 && m <= d.n2 ? (u64)d.Dc[m - 1] : 0;
    const u64 q0 = j >= 0 && j < d.n2 ? d.Dl[j] : 0;
    const u64 q1 = j >= 1 && j <= d.n2 ? (u64)d.Dc[j - 1] : 0;
    u64 lo = rv, t;
    int hi = 0;
    hi += add_ovf(lo, p0, &t) ? 1 : 0;
    lo = t;
    hi += add_ovf(lo, p1, &t) ? 1 : 0;
    lo = t;
    hi -= lo < q0 ? 1 : 0;
    lo -= q0;
    hi -= lo < q1 ? 1 : 0;
    lo -= q1;
    *plo = lo;
    *phi = hi;
}

// k_sdedge: one thread per chain block b, and one more for the ticket counter: the overflow of the
// limb below block b from the combine's d_r -- k_sdfix works in place, and by the time block b runs,
// block b - 1 may have overwritten that limb -- and the chain's flags and ticket cleared on the stream.
__global__ __launch_bounds__(256) void k_sdedge(SdArgs d, const u64 *r)
{
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b > d.nb) return;
    d.st[b] = 0;
    if (b == d.nb) return;
    int h = 0;
    if (b > 0) {
        const long m = b * SDFIX_CB - 1;
        u64 lo;
        sd_limb(d, m, r[m], &lo, &h);
    }
    d.edge[b] = h;
}

// k_sdfix: r <- r + D - (D << 64 n1) over `total` limbs.  A block takes a ticket, forms its
// SDFIX_CB limbs' sums with coalesced loads (limb base + k NT + t), hands them through LDS to the
// threads that own 8 consecutive limbs, and runs fold.hpp's signed chain (cf_chain_block: transfer
// functions, wave and workgroup scan, decoupled look-back), which stores the resolved limbs.  The
// carry out of the top limb is dropped: the result is the value mod 2^(64 total).
__global__ __launch_bounds__(SDFIX_NT) void k_sdfix(SdArgs d, u64 *r)
{
    constexpr int NT = SDFIX_NT, V = 8, CB = SDFIX_CB, NW = NT / 64;
    __shared__ u64 Lx[CB];
    __shared__ signed char Hs[CB];
    __shared__ int H[NT + 1];
    __shared__ u32 WF[NW];
    __shared__ u32 sh_b;
    __shared__ int sh_cin;
    const int t = threadIdx.x;
    if (t == 0) sh_b = __hip_atomic_fetch_add(&d.st[d.nb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const long b = sh_b;   // ticket: every block below it has started
    if (b >= d.nb) return;
    const long total = d.total, base = b * CB;
    u64 rv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const long m = base + k * NT + t;
        rv[k] = m < total ? r[m] : 0;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const long m = base + k * NT + t;
        u64 lo = 0;
        int hi = 0;
        if (m < total) sd_limb(d, m, rv[k], &lo, &hi);
        Lx[k * NT + t] = lo;
        Hs[k * NT + t] = (signed char)hi;
    }
    if (t == 0) H[0] = d.edge[b];
    __syncthreads();
    u64 lo[V];
    int hi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        lo[k] = Lx[t * V + k];
        hi[k] = Hs[t * V + k];
    }
    H[t + 1] = hi[V - 1];
    __syncthreads();
    cf_chain_block<NT>(lo, hi, H, WF, sh_cin, Lx, d.st, b, base, total, t, t & 63, t >> 6, r);
}
