// negaw.hpp -- products mod M = 2^B + 1 with the low-word CRT (the reference's fft_naive_convolution_1
// and the fix-up loop of FFT_mulmod_2expp1, mul_fft.c): the negacyclic top level of
// nega.hpp with pieces of up to N / 2 + 15 bits.  The transform gives c~_k = c_k mod p, p = 2^N + 1;
// the same convolution of the pieces' low 32-bit words, in wrapping 32-bit arithmetic, gives
// d_k = c_k mod 2^32.  p == 1 (mod 2^32), so t_k = (d_k - c~_k) mod 2^32 read as a signed int32 is
// floor(c_k / p) while |c_k| < 2^(N + 31), and c_k = c~_k + t_k p.
//   k_nlowconv       d = the length-2n negacyclic convolution mod 2^32 of the operands' piece low words
//   k_nwrapw<V>      the scratch sum T of the canonical coefficients (k_combine1) plus the words
//                    t_j (2^N + 1) 2^(j bits1), folded mod M: k_nwrap's chain (nega_chain), then k_nfix
#pragma once
#include "nega.hpp"

// --------------------------------------------------------------------------
// The low-word convolution.  Piece j's low word is bits [j bits1, j bits1 + 32) of the operand
// (bits1 >= 32), piece 0's minus the top limb (2^B == -1: the operand 2^B gives 0xFFFFFFFF).
// d_k = sum_i x_i s y_((k - i) mod 2n), s = -1 where k - i < 0.  A workgroup owns LC_TK outputs
// (blockIdx.x) and `ichunks` chunks of LC_TI terms i (blockIdx.y); per chunk the x_i and the signed
// partner window y_(k - i) go to LDS, each thread keeps LC_R outputs LC_NT apart in registers (its
// LDS reads run along consecutive words: no bank conflicts; x_i is a broadcast), and the partial
// sums are added to d with atomics (wrapping adds commute: the result does not depend on the
// order).  d is cleared before the launch.
// --------------------------------------------------------------------------
constexpr int LC_NT = 256, LC_R = 4, LC_TK = LC_NT * LC_R, LC_TI = 256;

struct LowConvArgs {
    const u64 *src[2];   // the operands, L + 1 limbs each (the same pointer twice: a square)
    long L;
    u64 bits1;
    long len;            // 2n
    u32 *d;              // len words
    int ichunks;         // chunks of LC_TI terms per workgroup
};

__device__ __forceinline__ u32 nega_lowword(const u64 *a, long L, u64 bits1, long j)
{
    const u64 pos = (u64)j * bits1;
    const long q = (long)(pos >> 6);
    const int sh = (int)(pos & 63);
    u64 v = a[q] >> sh;
    if (sh > 32 && q + 1 < L) v |= a[q + 1] << (64 - sh);
    u32 x = (u32)v;
    if (j == 0) x -= (u32)a[L];
    return x;
}

__global__ __launch_bounds__(LC_NT) void k_nlowconv(LowConvArgs a)
{
    __shared__ __attribute__((aligned(16))) u32 xs[LC_TI];
    __shared__ u32 ys[LC_TK + LC_TI];
    const int t = threadIdx.x;
    const long k0 = (long)blockIdx.x * LC_TK;
    u32 acc[LC_R];
#pragma unroll
    for (int r = 0; r < LC_R; ++r) acc[r] = 0;
    for (int c = 0; c < a.ichunks; ++c) {
        const long i0 = ((long)blockIdx.y * a.ichunks + c) * LC_TI;
        if (i0 >= a.len) break;   // the whole workgroup
        __syncthreads();
        xs[t] = i0 + t < a.len ? nega_lowword(a.src[0], a.L, a.bits1, i0 + t) : 0u;
        // ys[e]: the signed partner at k - i = mb + e (0 outside (-2n, 2n): only a k or an i past the end reads it)
        const long mb = k0 - i0 - (LC_TI - 1);
        for (int e = t; e < LC_TK + LC_TI - 1; e += LC_NT) {
            const long m = mb + e;
            u32 v = 0;
            if (m > -a.len && m < a.len) {
                v = nega_lowword(a.src[1], a.L, a.bits1, m < 0 ? m + a.len : m);
                if (m < 0) v = 0u - v;
            }
            ys[e] = v;
        }
        __syncthreads();
        // output k0 + t + r LC_NT, term i0 + ii: k - i - mb = t + r LC_NT + LC_TI - 1 - ii
#pragma unroll 4
        for (int ii = 0; ii < LC_TI; ii += 4) {
            const uint4 x4 = *(const uint4 *)&xs[ii];
#pragma unroll
            for (int r = 0; r < LC_R; ++r) {
                const u32 *y = &ys[t + r * LC_NT + LC_TI - 1 - ii];
                acc[r] += x4.x * y[0] + x4.y * y[-1] + x4.z * y[-2] + x4.w * y[-3];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < LC_R; ++r) {
        const long k = k0 + t + r * LC_NT;
        if (k < a.len) atomicAdd(&a.d[k], acc[r]);
    }
}

// --------------------------------------------------------------------------
// The fold.  With t_j as above and e_j = 1 where c~_j = 2^N (top = 1, limbs 0: k_combine1 leaves
// that 2^N out of T),
//   r == T + sum_j e_j 2^(N + j bits1) + sum_j t_j (2^N + 1) 2^(j bits1)   (mod M).
// The signed words enter with a fixed bias: u_j = t_j + 2^31 in [0, 2^32), formed on the fly as
// (d_j - low word of slot j) ^ 2^31, and the constant 2^31 at every j is taken off again.  As
// bits1 >= 32 the 32-bit words of one family do not overlap: W = sum_j u_j 2^(j bits1),
// C = sum_j 2^(31 + j bits1) and E = sum_j e_j 2^(j bits1) are all below 2^B, and
//   r == T + W + 2^N W + 2^N E - C - 2^N C.
// Every term is cut into B-bit pieces, piece i weighing (-1)^i, as in k_nwrap:
//   T_i       limbs [i L, (i + 1) L) of T                  sign (-1)^i
//   W         bits [0, B) of W                              sign +
//   Wb_q, Eb_q  bits [q B - N, (q + 1) B - N) of W, of E    sign (-1)^q
//   C         bits [0, B) of C                              sign -
//   Cb_q      bits [q B - N, (q + 1) B - N) of C            sign -(-1)^q
// A negative piece X enters as its B-bit complement, -X == ~X + 2 (mod M); K is twice their number.
// --------------------------------------------------------------------------
struct NegaWCombArgs {
    NegaCombArgs b;      // k_nwrap's (K: this fold's)
    const u32 *d;        // the low-word convolution, 2n words
};

__device__ __forceinline__ void nega_limbw(const NegaWCombArgs &aw, long m, u64 *lo, u32 *hi)
{
    const NegaCombArgs &a = aw.b;
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
    // bits [X, X + 64) of sum_j word(j) 2^(j bits1), 32-bit words (X may be below 0 or past B)
    auto window = [&](i64 X, auto word) {
        u64 v = 0;
        long j = X >= 32 ? udiv_inv((u64)(X - 32), a.bits1, a.inv_bits1) + 1 : 0;   // the first j bits1 > X - 32
        for (; j < a.len; ++j) {
            const i64 s = (i64)((u64)j * a.bits1) - X;   // in (-32, 64)
            if (s >= 64) break;
            if (s <= -32) continue;   // (a start one early)
            const u64 wv = word(j);
            v |= s >= 0 ? wv << s : wv >> -s;
        }
        return v;
    };
    auto wu = [&](long j) { return (u64)((aw.d[j] - (u32)a.dig[(size_t)j * a.l]) ^ 0x80000000u); };
    auto we = [&](long j) { return (u64)(a.top[j] != 0); };
    auto wc = [&](long) { return (u64)0x80000000u; };
    const i64 P = (i64)m * 64, B = (i64)a.L * 64;
    add(window(P, wu));
    add(~window(P, wc));
    for (int q = 0; q <= a.qmax; ++q) {
        const i64 X = P + (i64)q * B - (i64)a.N;
        const u64 vu = window(X, wu), ve = window(X, we), vc = window(X, wc);
        add(q & 1 ? ~vu : vu);
        add(q & 1 ? ~ve : ve);
        add(q & 1 ? vc : ~vc);
    }
    if (m == 0) add((u64)a.K);
    *lo = slo;
    *hi = shi;
}

template <int V>
__global__ __launch_bounds__(256) void k_nwrapw(NegaWCombArgs a, u64 *r, u32 *st)
{
    nega_chain<V>(a.b.L, a.b.nblk, [&](long m, u64 *lo, u32 *hi) { nega_limbw(a, m, lo, hi); }, r, st);
}
