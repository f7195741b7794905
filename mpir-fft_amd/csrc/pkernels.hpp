// pkernels.hpp -- sub-quadratic pointwise products mod p = 2^N + 1 for big coefficients
// (the nested negacyclic transform of FFT_mulmod_2expp1 /
// fft_mulmod_2expp1, mul_fft.c:2998-3167, FFT/IFFT_radix2_negacyclic :1290, :1861).
//
// One workgroup computes one product a b mod p (a, b in the reduced HBM form, N = 64 l bits):
//   * a, b are cut into K = 2^lk pieces of B = N/K bits (thread t owns piece t);
//   * the negacyclic convolution of the pieces (X^K == -1 with X = 2^B, so it IS the
//     product mod p) is computed in the inner ring R' = Z/(2^N' + 1), N' = 64 M, with
//     N' >= 2B + lk + 4 so every signed convolution coefficient |c_t| < K 2^(2B+2) is
//     recovered exactly from its residue (the reference instead restores the top
//     with a naive convolution of the low limbs, :3088; headroom is cheaper here);
//   * negacyclic weights theta^t, theta = 2^(N'/K) a 2K-th root of unity, then a length-K
//     cyclic DIF transform with root omega = theta^2 = 2^(2N'/K), pointwise products in R',
//     DIT inverse, division by K and un-weighting.  Only omega must be a power of two:
//     N' is a multiple of K/2 (not K), and when N'/K is a half-integer the odd weights use
//     sqrt(2) = 2^(N'/4) (2^(N'/2) - 1) in R' (pw_sqrt2, one in-thread half swap) -- the
//     identity of the reference's FFT_radix2_butterfly_sqrt2 (mul_fft.c:580-640) applied to the inner
//     ring.  That lets N' be the smallest multiple of 64 K/2 bits above the headroom bound
//     (C3: 1152 instead of 1280 bits, C4: 1280 instead of 1536).
//   All the other multiplications are by powers of two.
// Thread t holds its coefficient (M limbs + a small signed top word, value =
// limbs + top 2^N') in registers: additions are in-thread carry chains
// (v_add_co / v_addc).  A butterfly partner is read from LDS (limb-major,
// conflict-free) already rotated by the relative exponent; each thread keeps a
// *pending* exponent so its own value is never rotated.  The inner products are
// in-thread product-scanning on 29/30-bit digits (v_mad_u64_u32): schoolbook, or one
// Karatsuba level over the N'/2 halves whose fold by 2^N' == -1 is part of the
// recombination (pw_mulmod; a per-M compile-time switch, pw_kara).
// The coefficients are then summed (with their signs and the negacyclic wrap) into
// the l output limbs and stored in the reduced HBM form the inverse pass loads.
#pragma once
#include <type_traits>
#include "coeff.hpp"

// LDS of one k_pwss workgroup: M K limbs (the exchange rows, then the coefficients; the l
// output overflows alias them) + three more exchange rows of K words (rows 2M .. 2M+2: the
// complements of rows 0 .. 2, pw_group) + one K-word array of tops and pending exponents
// (pw_pack_tp).  C3 (M = 18, K = 256): 40 960 B, exactly a quarter of a CU's 160 KiB, so four
// workgroups share it (pw_wpe).
// Tight form (K = 512): no top / pending-exponent arrays beside the exchange rows --
// a level's partner tops and exponents go by a wave shuffle (partner in the wave) or through
// the first two exchange rows before the words are published (two more barriers), and the
// signed coefficients are stored as two's complement (no sign array) -- so the workgroup needs
// exactly M K 8 bytes: 80 KiB at C4 (M = 20), two workgroups per CU instead of one (the round-3
// form took 86 KB, one workgroup per CU).
__host__ __device__ constexpr bool pw_tight(int K) { return K == 512; }
// operand B's pieces loaded after A's forward transform (pw_slot_product's loadB): the tight
// form only (C4 pointwise 39.0 -> 37.7 ms; at l = 2048, four workgroups per CU, 0.5-2 % slower:
// profiles/r04/pw_tight_ab.txt)
__host__ __device__ constexpr bool pw_late_b(int K) { return pw_tight(K); }
// inputs in flight in the late operand-B quad loader: one (A's transformed limbs are live; with two
// the C4 kernel spilled 40 B per lane, with one it has no scratch at all, at equal speed:
// C4 pointwise 32.41 vs 32.49 ms, profiles/r05/pw_late_infl_ab.txt); in operand A's: two
constexpr int pw_late_infl = 1, pw_a_infl = 2;

// Grouped wrap selects (pw_combine GRP): the exchange has GRP - 1 rows more, rows 2M .. 2M+GRP-2
// = ~rows 0 .. GRP-2, so a reader takes the wrap test, the base select and the mask select once
// per GRP consecutive words (6 VALU per word -> 4.5 at GRP = 2 -> 3.75 at GRP = 4).  Not in the
// tight form: its 80 KiB have no room for a row, it keeps the per-word form.  GRP = 4 (three rows)
// fits four workgroups per CU only with the tops and pending exponents packed into one K-word
// array (pw_pack_tp).  C3, ms per multiply: 7.13-7.16 per word, 6.85-6.90 in pairs, 6.78-6.80 in
// fours (profiles/r12/pw_pair_ab.txt).
__host__ __device__ constexpr int pw_group(int K) { return pw_tight(K) ? 1 : 4; }
// tops and pending exponents in one word per thread, (2 T + S) << 12 | P  (P < 2 N' < 2^12; the
// tops are a few units: pw_norm, pw_sqrt2)
__host__ __device__ constexpr bool pw_pack_tp(int K) { return !pw_tight(K); }
// 32-bit words of the exchange rows ahead of the packed tops and pending exponents (TT)
__host__ __device__ constexpr size_t pw_row_words(int M, int K) { return (size_t)(2 * M + pw_group(K) - 1) * K; }

__host__ __device__ constexpr size_t pw_lds_bytes(int M, int K, int l)
{
    return (pw_row_words(M, K) * 4 > (size_t)l * 4 ? pw_row_words(M, K) * 4 : (size_t)l * 4) +
           (pw_pack_tp(K) ? (size_t)K * 4 : 0);
}
// the shipped shapes (pw_wpe): a quarter of a CU's 160 KiB at C3, half at C4
static_assert(pw_lds_bytes(10, 256, 1024) == 24576, "M = 10, K = 256, l = 1024");
static_assert(pw_lds_bytes(18, 256, 2048) == 40960, "M = 18, K = 256, l = 2048");
static_assert(pw_lds_bytes(20, 512, 4096) == 81920, "M = 20, K = 512, l = 4096");

// waves per SIMD k_pwss is compiled for: 4 (VGPRs <= 128) where the LDS fits 1024 threads per
// CU (K = 256: four workgroups; the tight K = 512 form: two), else 2 (the compiler's choice,
// ~140-170 VGPRs)
template <int M, int LK>
__host__ __device__ constexpr int pw_wpe()
{
    return pw_lds_bytes(M, 1 << LK, 64 * M) * (1024 >> LK) <= 160 * 1024 ? 4 : 2;
}
// partner-word prefetch distance of pw_combine for that budget: 14 words in flight.  With 16 and
// pw_canon's branch (below) k_pwss<18,8,*> parked 5-12 words of operand B in scratch across A's
// transform; 14 has no scratch in any instance and measured no slower (C3 6.729 against 6.777 ms
// with 16, 6.717 with 12; C4 68.43 against 68.56: profiles/r17/pw_chain_ab.txt)
#ifndef PW_PDW
#define PW_PDW 14   // A/B builds
#endif
template <int M, int LK>
__host__ __device__ constexpr int pw_pd() { return pw_wpe<M, LK>() == 4 ? PW_PDW : 2 * M; }

// Exchange format: thread t publishes its value as 2M 32-bit words, word k at
// Xw[k K + t] (conflict-free for any rotation), top in TT[t]; where pw_group(K) = G > 1, also the
// complements of words 0 .. G-2 at rows 2M .. 2M+G-2.  Before publishing,
// pw_norm moves the top to -1 (almost always exactly): the reader's rotation then
// needs no correction term, only a complement mask and one carry chain.

// L + T 2^N' == (L - (T + 1)) - 2^N'  (mod p'): subtract D = T + 1; returns the new top
// (-1 unless the subtraction left [0, 2^N'), which needs L < D or L - D >= 2^N').
// PW_NORM_SPILL_ALL (test builds only, libmpfft_pwspill.so): every lane takes the device form's
// rare branch below -- keeps its top -- so the readers' T_q != -1 path runs on every exchange
// (tests/test_gpu_parity.py::test_pointwise_norm_spill_branch)
#ifndef PW_NORM_SPILL_ALL
#define PW_NORM_SPILL_ALL 0
#endif
template <int M>
__host__ __device__ __forceinline__ int pw_norm(u64 (&L)[M], int T)
{
    const int D = T + 1;
#if defined(__HIP_DEVICE_COMPILE__)
    // Device form (the kernel is VALU-bound): a small D only moves the low word unless it
    // under/overflows (probability ~2^-32 per lane); such a lane keeps its top, which every
    // reader handles (pw_combine's Tq != -1 branch) -- no full chain, whose rewrite of all M
    // limbs under a branch made the compiler keep a second copy of L live across the levels'
    // loop and spill it there (C4 pointwise 34.9 -> 34.1 ms, C3 3.47 -> 3.43 ms)
    {
        const u32 w0 = (u32)L[0], n0 = w0 - (u32)D;
        const bool spill = PW_NORM_SPILL_ALL || (D > 0 ? w0 < (u32)D : (D < 0 ? n0 < (u32)(-D) : false));
        L[0] = (L[0] & ~0xffffffffull) | (spill ? w0 : n0);
        return spill ? T : -1;
    }
#endif
    const u32 dh = D < 0 ? ~0u : 0u;
    u32 b = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const u32 lo = __builtin_subc((u32)L[j], j == 0 ? (u32)D : dh, b, &b);
        const u32 hi = __builtin_subc((u32)(L[j] >> 32), dh, b, &b);
        L[j] = ((u64)hi << 32) | lo;
    }
    // L - D = L' + ((D < 0) - b) 2^N'
    return (D < 0) - (int)b - 1;
}

// Values are kept with a sign flag S: the represented value is (-1)^S (L + T 2^N'), so
// a butterfly's "-own" is a flag flip and every combine is own + (+-) rotated partner,
// the partner's sign folded into the complement mask.
// r = alpha * own + 2^E * x_q  (mod p', not reduced); alpha in {-1, 0, 1}.
// x_q: words Xw[k K + q], TT[q] = 2 T_q + S_q.  With E' = E mod N' = 32 Yw + s5, s5 in [1, 32]:
//   out = the N'-bit circular rotation of x_q's limbs by E', its low E' (wrapped) bits
//         complemented:  out_k = alignbit(w_k, w_(k-1), 32 - s5),
//         w_i = Xw[(i - Yw) mod 2M], complemented when i < Yw (i in [-1, 2M));
//   2^E' x_q == out + 1 - (1 + T_q) 2^E'   (rotation wraps negated; T_q 2^N' == -T_q);
//   negated (E >= N', or the signs differ):  ~out + 1 + (1 + T_q) 2^E'.
// After pw_norm T_q = -1 on all but ~2^-32 of the lanes (a lane whose low word would under- or
// overflow keeps its top, pw_norm's device form), so the (1 + T_q) term is a rare branch, and the
// whole sum is one add-with-carry chain with carry-in 1.
// packed: the partner's 2 T_q + S_q (TT[q], or a register in the tight form)
// FIXE >= 0: the caller guarantees E mod N' == FIXE, so the rotation is a compile-time constant
// and every wrap test, word address and complement mask below folds away (the forward
// transforms' first level, where E is exactly N'/2 for every thread: pw_transform)
// GRP = 2: the caller guarantees row 2M of the partner's column holds ~w_0 (pw_publish_words where
// pw_group(K) = 2).  Words k, k + 1 (k even) then share the wrap test of k: in stream order the pair
// straddles the wrap only when k + 1 == Yw, its second word is row 0 read plain -- which is row
// 2M (same base as row 2M - 1) under the wrapped mask, ~w_0 ^ ~smask = w_0 ^ smask.  One compare
// and two selects per pair instead of per word; w_(-1) stays on its own.  GRP = 4: the same with
// rows 2M .. 2M+2 = ~w_0 .. ~w_2 and words k .. k + 3 (k a multiple of 4) sharing the test of k.
template <int M, int LK, int PD = 2 * M, int FIXE = -1, int GRP = 1>
__host__ __device__ __forceinline__ void pw_combine(u64 (&L)[M], int &T, int &S, int alpha, const u32 *Xw,
                                                   int packed, int q, unsigned E)
{
    constexpr int K = 1 << LK, NW = 2 * M;
    constexpr unsigned NP = 64 * M;
    static_assert(GRP == 1 || GRP == 2 || GRP == 4, "group sizes built");
    const int Tq = packed >> 1, Sq = packed & 1;
    bool neg = E >= NP;
    if (neg) E -= NP;
    if (FIXE >= 0) E = (unsigned)FIXE;
    const int Yw = ((int)E - 1) >> 5;                    // E = 0: Yw = -1, s5 = 32
    const unsigned sh = (unsigned)(32 * (Yw + 1)) - E;   // 32 - s5, in [0, 31]
    if (alpha == 0) {
#pragma unroll
        for (int j = 0; j < M; ++j) L[j] = 0;
        T = 0;
        S = 0;
    } else if (alpha < 0) {
        S ^= 1;
    }
    neg ^= (S ^ Sq) != 0;
    const u32 smask = neg ? ~0u : 0u;
    const u32 *bn = Xw + q - Yw * K;          // source word i >= Yw: bn[i K]
    const u32 *bw = bn + NW * K;              // i < Yw: wrapped
    // w_(-1): wrapped unless Yw = -1 (then it is word 0 and the funnel shift is 0).
    // Yw = -1 also reads row 2M at k = 2M - 1 (unused by the funnel): the buffer has it.
    u32 wprev = (-1 < Yw ? bw : bn)[-K] ^ (-1 < Yw ? ~smask : smask);
    u32 c = 1;
    // partner words are read PD ahead of their use: all NW at once by default (one or two
    // at a time, the compiler's own order, exposed the LDS latency per word); a bounded
    // distance where the kernel must fit 128 VGPRs (pw_wpe: more waves hide the latency)
    constexpr int D0 = PD < NW ? PD : NW;
    u32 wv[NW];
#pragma unroll
    for (int k = 0; k < D0; ++k) {
        const bool wr = (k & ~(GRP - 1)) < Yw;
        wv[k] = (wr ? bw : bn)[k * K];
#if defined(__HIP_DEVICE_COMPILE__)
        if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
#endif
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        if (k + D0 < NW) {
            const bool wr2 = ((k + D0) & ~(GRP - 1)) < Yw;
            wv[k + D0] = (wr2 ? bw : bn)[(k + D0) * K];
        }
        const bool wr = (k & ~(GRP - 1)) < Yw;
        const u32 w = wv[k] ^ (wr ? ~smask : smask);
#if defined(__HIP_DEVICE_COMPILE__)
        const u32 o = __builtin_amdgcn_alignbit(w, wprev, sh);
#else
        const u32 o = (u32)((((u64)w << 32) | wprev) >> sh);
#endif
        wprev = w;
        const u32 lw = (u32)(L[k >> 1] >> (32 * (k & 1)));
        const u32 r = __builtin_addc(lw, o, c, &c);
        if (k & 1) L[k >> 1] = (L[k >> 1] & 0xffffffffull) | ((u64)r << 32);
        else L[k >> 1] = (L[k >> 1] & ~0xffffffffull) | r;
#if defined(__HIP_DEVICE_COMPILE__)
        if (D0 < NW && (k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
#endif
    }
    T += (int)c;
    if (Tq != -1) {   // rare: add cv 2^E', cv = -(1 + T_q) (negated when E >= N')
        const int cv = neg ? 1 + Tq : -1 - Tq;
        const i64 d = (i64)cv * ((i64)1 << (32 - sh));
        const u32 dl = (u32)d, dhi = (u32)((u64)d >> 32), sx = d < 0 ? ~0u : 0u;
        u32 cc = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const u32 ad = k < Yw ? 0u : k == Yw ? dl : k == Yw + 1 ? dhi : sx;
            const u32 lw = (u32)(L[k >> 1] >> (32 * (k & 1)));
            const u32 r = __builtin_addc(lw, ad, cc, &cc);
            if (k & 1) L[k >> 1] = (L[k >> 1] & 0xffffffffull) | ((u64)r << 32);
            else L[k >> 1] = (L[k >> 1] & ~0xffffffffull) | r;
        }
        T += (int)cc + (Yw == NW - 1 ? (int)(d >> 32) : (d < 0 ? -1 : 0));
    }
}

// canonical residue of L + T 2^N' (== L - T): limbs in [0, 2^N'), returns 1 for 2^N' (L = 0)
// The limbs are below 2^N' < p' as they stand, so a small T only moves the low word unless that
// word under- or overflows (~2^-32 per lane, as in pw_norm's device form): then L - T is the
// residue and the flag is 0.  Only a lane whose low word wraps takes the two folds below (a
// branch the wave skips otherwise); with PW_NORM_SPILL_ALL every lane does.  One form for the
// host and the device.
// FAST = false: the two folds on every lane, no branch.  The K = 256 kernels sit at their 128
// VGPRs through the forward transforms, and a branch here that rewrites all M limbs changes what
// the register allocator evicts there: with the branch at operand B's pw_canon as well,
// k_pwss<18,8,0> parked 2 words of B's pieces in scratch across A's transform and k_pwss<20,9,0>
// 3; with it at A's in the cached tight form, k_pwsp<20,9,*> 2 (profiles/r17/pw_chain_isa.txt).
// Those two sites keep the plain form.
template <bool PRE>
__host__ __device__ constexpr bool pw_canon_fast_a(int K) { return !(PRE && pw_tight(K)); }
template <int M, bool FAST = true>
__host__ __device__ __forceinline__ int pw_canon(u64 (&L)[M], int T)
{
    if (FAST) {
        const u32 w0 = (u32)L[0], n0 = w0 - (u32)T;
        const bool wrap = PW_NORM_SPILL_ALL || (T > 0 ? w0 < (u32)T : (T < 0 ? n0 < 0u - (u32)T : false));
        L[0] = (L[0] & ~0xffffffffull) | (wrap ? w0 : n0);
        if (__builtin_expect(!wrap, 1)) return 0;
    }
    // L - T = L' + c1 2^N' == L' - c1 (|c1| <= 1), then L' - c1 = L'' + c2 2^N': two 32-bit chains
    // over the words, each adding a small constant sign-extended; c2 != 0: the second fold wrapped,
    // the value is 2^N' == -1
    int cf = -T;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const u32 sx = cf < 0 ? ~0u : 0u;
        u32 c = 0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const u32 lo = __builtin_addc((u32)L[j], j == 0 ? (u32)cf : sx, c, &c);
            const u32 hi = __builtin_addc((u32)(L[j] >> 32), sx, c, &c);
            L[j] = ((u64)hi << 32) | lo;
        }
        cf = -((int)c - (cf < 0 ? 1 : 0));
    }
    const u64 keep = cf != 0 ? 0ull : ~0ull;
#pragma unroll
    for (int j = 0; j < M; ++j) L[j] &= keep;
    return cf != 0;
}

// L + T 2^N'  <-  (2^(N'/2) - 1) (L + T 2^N')  mod p'  (M even; lo, hi = the low and high
// M/2 limbs of L):  2^(N'/2) (lo + hi 2^(N'/2) + T 2^N') == lo 2^(N'/2) - hi - T 2^(N'/2), so
// the product is (T - hi - lo) + (lo - hi - T) 2^(N'/2).  Each half is two 32-bit borrow chains
// (T sign-extended over the half's words): (T - hi) - lo and (lo - hi) - T, the four run word by
// word side by side, so that every v_subb has the other three between it and the next of its own
// chain (gfx950: two wait states from a VALU's carry out to the VALU that reads it).  The low
// half's carry a0 (in [-3, 0]) goes into the high half: into its low word alone unless that word
// underflows (~2^-32 per lane), else rippled through the half.  The new top is small
// (|T'| <= |T| + 3).
template <int M>
__host__ __device__ __forceinline__ void pw_sqrt2(u64 (&L)[M], int &T)
{
    static_assert(M % 2 == 0, "the half swap needs an even limb count");
    constexpr int H = M / 2;
    const u32 tx = T < 0 ? ~0u : 0u;
    u32 b1 = 0, b2 = 0, b3 = 0, b4 = 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const u64 lo = L[j], hi = L[j + H];
        u32 r[2], s[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u32 lw = (u32)(lo >> (32 * e)), hw = (u32)(hi >> (32 * e)), tw = j == 0 && e == 0 ? (u32)T : tx;
            r[e] = __builtin_subc(__builtin_subc(tw, hw, b1, &b1), lw, b2, &b2);
            s[e] = __builtin_subc(__builtin_subc(lw, hw, b3, &b3), tw, b4, &b4);
        }
        L[j] = ((u64)r[1] << 32) | r[0];
        L[j + H] = ((u64)s[1] << 32) | s[0];
    }
    // T - hi - lo = low half + a0 2^(N'/2);  lo - hi - T = high half + a1 2^(N'/2)
    const int a0 = (T < 0 ? -1 : 0) - (int)b1 - (int)b2, a1 = (T < 0 ? 1 : 0) - (int)b3 - (int)b4;
    const u32 h0 = (u32)L[H], d0 = 0u - (u32)a0;   // a0 <= 0
    const bool wrap = h0 < d0;
    L[H] = (L[H] & ~0xffffffffull) | (wrap ? h0 : h0 - d0);
    T = a1;
    if (__builtin_expect(wrap, 0)) {   // rare: a0 < 0 borrows out of the high half's low word
        u32 c = 0;
#pragma unroll
        for (int j = H; j < M; ++j) {
            const u32 lw = __builtin_addc((u32)L[j], j == H ? (u32)a0 : ~0u, c, &c);
            const u32 hw = __builtin_addc((u32)(L[j] >> 32), ~0u, c, &c);
            L[j] = ((u64)hw << 32) | lw;
        }
        T = a1 + (int)c - 1;
    }
}

// The product's limbs go to `Z`: registers (u64 (&)[M]) or, on the device, this thread's word
// column of the LDS exchange rows (PwLdsZ: limb j as words 2j, 2j + 1) -- the latter keeps the M limbs out of the
// registers while the 2 ND digits are live (the l = 4096 kernel spilled 32 VGPRs at the
// 128-VGPR budget with the limbs in registers, the l = 2048 one 5).
struct PwLdsRef {
    u32 *p;    // word 0 of the limb (its high word K further): the publish layout (pw_publish_words)
    int K;
    __device__ __forceinline__ operator u64() const { return ((u64)p[K] << 32) | p[0]; }
    __device__ __forceinline__ PwLdsRef &operator=(u64 v)
    {
        p[0] = (u32)v;
        p[K] = (u32)(v >> 32);
        return *this;
    }
};
struct PwLdsZ {
    u32 *z;    // Xw + t: this thread's own word column (the u64 rows would straddle two threads' columns)
    int K;
    __device__ __forceinline__ PwLdsRef operator[](int j) const { return PwLdsRef{z + 2 * j * K, K}; }
};

// 32-bit word k of a product sink (registers or PwLdsZ): init writes the words in order (an even
// word first, so no limb is read before it is whole), put replaces one, get reads one
template <int M>
__host__ __device__ __forceinline__ void pw_zword_init(u64 (&Z)[M], int k, u32 w)
{
    if (k & 1) Z[k >> 1] |= (u64)w << 32;
    else Z[k >> 1] = w;
}
template <int M>
__host__ __device__ __forceinline__ void pw_zword_put(u64 (&Z)[M], int k, u32 w)
{
    if (k & 1) Z[k >> 1] = (Z[k >> 1] & 0xffffffffull) | ((u64)w << 32);
    else Z[k >> 1] = (Z[k >> 1] & ~0xffffffffull) | w;
}
template <int M>
__host__ __device__ __forceinline__ u32 pw_zword_get(const u64 (&Z)[M], int k) { return (u32)(Z[k >> 1] >> (32 * (k & 1))); }
__device__ __forceinline__ void pw_zword_init(const PwLdsZ &Z, int k, u32 w) { Z.z[k * Z.K] = w; }
__device__ __forceinline__ void pw_zword_put(const PwLdsZ &Z, int k, u32 w) { Z.z[k * Z.K] = w; }
__device__ __forceinline__ u32 pw_zword_get(const PwLdsZ &Z, int k) { return Z.z[k * Z.K]; }

// ---- Karatsuba over the N'/2 halves (pw_mulmod's main path where pw_kara<M>()) ----------------
// With X = 2^(N'/2), a = a0 + X a1, b = b0 + X b1 and X^2 = 2^N' == -1, three half products give
// the residue with the fold already done:
//   P0 = a0 b0,  P2 = a1 b1,  Ps = (a0 + a1)(b0 + b1),  a0 b1 + a1 b0 = Ps - P0 - P2
//   a b == (P0 - P2) + X (Ps - P0 - P2)
//       == [p0l + p0h - p2l + p2h - psh] + X [p0h - p0l - p2l - p2h + psl]      (mod 2^N' + 1)
// (pXl, pXh: the low N'/2 bits of a product and the rest).  The sums a0 + a1, b0 + b1 (one bit
// wider than a half, which the half's top digit has room for at every M here) instead of the
// differences: no signs, so no |.|, no conditional negate and no complement masks in the
// recombination.  3 ND_h^2 digit products instead of ND^2 (M = 18: 1 200 instead of 1 600).

// the M each form ships at: the form that measured faster; a compile-time switch
#ifndef PW_KARA_MASK
#define PW_KARA_MASK 1   // A/B builds: bit 0: M = 18, bit 1: M = 20, bit 2: M = 10
#endif
template <int M>
__host__ __device__ constexpr bool pw_kara()
{
    return M % 2 == 0 && ((M == 18 && (PW_KARA_MASK & 1)) || (M == 20 && (PW_KARA_MASK & 2)) || (M == 10 && (PW_KARA_MASK & 4)));
}
// digit width of the half products: the widest with ND_h 2^(2 DB) < 2^64 that saves a digit
template <int M>
__host__ __device__ constexpr int pw_kara_db() { return M == 10 ? 30 : 29; }

// Where the two half sums (2M words) wait while P0 and P2 are formed: this thread's own word
// column of the LDS exchange rows (PwParkLds; the rows are idle between the forward transforms'
// last in-wave level and the inverse's first publish, the argument of pw_slot_product's PwLdsZ
// branch), or registers (the host build, and callers without a column)
struct PwParkLds {
    u32 *z;    // Xw + t
    int K;
    __device__ __forceinline__ void put(int k, u32 w) { z[k * K] = w; }
    __device__ __forceinline__ u32 get(int k) const { return z[k * K]; }
};
template <int NW>
struct PwParkReg {
    u32 w[NW];
    __host__ __device__ __forceinline__ void put(int k, u32 v) { w[k] = v; }
    __host__ __device__ __forceinline__ u32 get(int k) const { return w[k]; }
};

// the ND DB-bit digits of the value whose 32-bit word i is word(i) (0 past its end)
template <int DB, int ND, typename W>
__host__ __device__ __forceinline__ void pw_digits(u32 (&d)[ND], W word)
{
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int b0 = i * DB, wi = b0 >> 5, sh = b0 & 31;
        u32 x = word(wi) >> sh;
        if (sh + DB > 32) x |= word(wi + 1) << (32 - sh);
        d[i] = x & ((1u << DB) - 1);
    }
}

// Half product: the low NW 32-bit words of (sum ad[i] 2^(DB i)) (sum bd[i] 2^(DB i)), product-
// scanning, handed to sink(k, word) in order k = 0 .. NW - 1 (registers, an add chain or an LDS
// column: the caller's choice).  A column's excess over its DB-bit digit is the 64-bit addend of
// the next column's first v_mad_u64_u32 (col >> DB), and the digits are packed into words as
// they appear: 4 VALU per column beside the products, where a 128-bit accumulator took 8.
// SQR: the square of ad's value, bd = 2 ad (the doubled digits): every off-diagonal product once,
// ND (ND + 1) / 2 products; with multiplicity a column still sums at most ND products.
template <int ND, int DB, int NW, bool SQR = false, typename Sink>
__host__ __device__ __forceinline__ void pw_halfprod(const u32 (&ad)[ND], const u32 (&bd)[ND], Sink &&sink)
{
    // carry-in < 2^(64 - DB) <= 2^(2 DB), at most ND products below 2^(2 DB) each
    static_assert(DB < 32 && 3 * DB >= 64 && (unsigned long long)(ND + 1) <= (1ull << (64 - 2 * DB)),
                  "column sums must stay below 2^64");
    constexpr int NPC = (32 * NW + DB - 1) / DB;   // DB-bit pieces that cover NW words
    u64 col = 0;
    u32 cur = 0;
#pragma clang loop unroll(full)
    for (int c = 0; c < NPC; ++c) {
        if (c <= 2 * ND - 2) {
            const int i0 = c < ND ? 0 : c - ND + 1, i1 = c < ND ? c : ND - 1;
            if (SQR) {
#pragma clang loop unroll(full)
                for (int i = i0; 2 * i < c; ++i) col += (u64)bd[i] * ad[c - i];
                if (!(c & 1)) col += (u64)ad[c / 2] * ad[c / 2];
            } else {
#pragma clang loop unroll(full)
                for (int i = i0; i <= i1; ++i) col += (u64)ad[i] * bd[c - i];
            }
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_sched_barrier(0);   // one column's products live at a time (VGPRs)
#endif
        }
        const u32 dg = (u32)col & ((1u << DB) - 1);
        col >>= DB;
        const int bits = (c * DB) & 31, k = (c * DB) >> 5;   // bits of word k already in cur
        cur = bits ? cur | (dg << bits) : dg;
        if (bits + DB >= 32) {
            if (k < NW) sink(k, cur);
            cur = dg >> ((32 - bits) & 31);   // (bits + DB >= 32 with DB < 32: bits > 0)
        }
    }
}

// The Karatsuba recombination's last step: Zw (2M words) + clo X + chi X^2, X = 2^(N'/2), with
// small signed clo, chi (|clo|, |chi| < 2^30) == Zw + (clo X - chi) mod p'.  One chain over the
// 2M words adds clo at word M and -chi at word 0 and leaves a top in {-1, 0, 1}; a top of 1 (the
// words are then small) is folded once more: Zw + 2^N' == Zw - 1, and Zw = 0 gives 2^N' - 1 with
// top -1.  Returns the top, in {-1, 0}: value == Zw + top 2^N'.
template <int M>
__host__ __device__ __forceinline__ int pw_kara_fold(u32 (&Zw)[2 * M], int clo, int chi)
{
    const int e0 = chi > 0 ? -1 : 0, d = clo + e0;   // -chi = its M low words + e0 X
    const u32 x0 = e0 ? ~0u : 0u, x1 = d < 0 ? ~0u : 0u;
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < 2 * M; ++k)
        Zw[k] = __builtin_addc(Zw[k], k == 0 ? (u32)(-chi) : k < M ? x0 : k == M ? (u32)d : x1, c, &c);
    int top = (int)c - (d < 0 ? 1 : 0);
    if (top > 0) {   // rare
        u32 b = 1;
#pragma unroll
        for (int k = 0; k < 2 * M; ++k) Zw[k] = __builtin_subc(Zw[k], 0u, b, &b);
        top = -(int)b;
    }
    return top;
}

// a b (SQR: a^2, Lb unused) mod p' for limbs below 2^N' by one Karatsuba level (above): the
// main path of pw_mulmod and pw_sqrmod where pw_kara<M>().  A square runs the same chains on
// three half squares, so pw_sqrmod(a) and pw_mulmod(a, a) return the same limbs and top.
template <int M, bool SQR, typename ZT, typename PK>
__host__ __device__ __forceinline__ void pw_kara_product(ZT &&Z, int &T, const u64 (&La)[M], const u64 (&Lb)[M], PK &park)
{
    // The order that keeps the register peak lowest: the half sums first, while La / Lb are
    // whole, and parked as words; P0 from the low halves into the result words, turned into
    // (p0l + p0h, p0h - p0l) as its high words appear (its digits die as the result grows); P2
    // from the high halves, then Ps from the parked sums, their words added and subtracted into
    // the two running chains as they are emitted.
    // All chains are 32-bit v_addc / v_subb with explicit carries.
    constexpr int DB = pw_kara_db<M>(), ND = (32 * M + 1 + DB - 1) / DB;   // digits of a half sum
    static_assert(ND == (32 * M + DB - 1) / DB, "the half sums' extra bit must not cost a digit");
    auto wa = [&](int i) -> u32 { return (u32)(La[i >> 1] >> (32 * (i & 1))); };
    auto wb = [&](int i) -> u32 { return (u32)(Lb[i >> 1] >> (32 * (i & 1))); };
    u32 sca = 0, scb = 0;   // the sums' bit N'/2
#pragma unroll
    for (int k = 0; k < M; ++k) {
        park.put(k, __builtin_addc(wa(k), wa(M + k), sca, &sca));
        if (!SQR) park.put(M + k, __builtin_addc(wb(k), wb(M + k), scb, &scb));
    }
    u32 ad[ND], bd[ND];
    // the second factor's digits: b's, or for a square the doubled digits of a (pw_halfprod SQR)
    auto second = [&](auto word) {
        if constexpr (SQR) {
#pragma unroll
            for (int i = 0; i < ND; ++i) bd[i] = 2 * ad[i];
        } else {
            pw_digits<DB, ND>(bd, word);
        }
    };
    u32 Zw[2 * M];   // words 0 .. M-1: the low chain, M .. 2M-1: the high chain
    int clo = 0, chi = 0;   // their signed carries (weights 2^(N'/2), 2^N' over the chain's base)
    pw_digits<DB, ND>(ad, [&](int i) -> u32 { return i < M ? wa(i) : 0u; });
    second([&](int i) -> u32 { return i < M ? wb(i) : 0u; });
    {
        u32 c = 0, b = 0;
        pw_halfprod<ND, DB, 2 * M, SQR>(ad, bd, [&](int k, u32 w) {
            if (k < M) {
                Zw[k] = w;
            } else {
                const u32 lo = Zw[k - M];
                Zw[k - M] = __builtin_addc(lo, w, c, &c);   // p0l + p0h
                Zw[k] = __builtin_subc(w, lo, b, &b);       // p0h - p0l
            }
        });
        clo += (int)c;
        chi -= (int)b;
    }
    pw_digits<DB, ND>(ad, [&](int i) -> u32 { return i < M ? wa(M + i) : 0u; });
    second([&](int i) -> u32 { return i < M ? wb(M + i) : 0u; });
    {
        u32 b1 = 0, b2 = 0, c3 = 0, b4 = 0;
        pw_halfprod<ND, DB, 2 * M, SQR>(ad, bd, [&](int k, u32 w) {
            if (k < M) {   // - p2l in both
                Zw[k] = __builtin_subc(Zw[k], w, b1, &b1);
                Zw[M + k] = __builtin_subc(Zw[M + k], w, b2, &b2);
            } else {       // + p2h low, - p2h high
                Zw[k - M] = __builtin_addc(Zw[k - M], w, c3, &c3);
                Zw[k] = __builtin_subc(Zw[k], w, b4, &b4);
            }
        });
        clo += (int)c3 - (int)b1;
        chi -= (int)b2 + (int)b4;
    }
    pw_digits<DB, ND>(ad, [&](int i) -> u32 { return i < M ? park.get(i) : i == M ? sca : 0u; });
    second([&](int i) -> u32 { return i < M ? park.get(M + i) : i == M ? scb : 0u; });
    {
        u32 c = 0, b = 0;   // Ps < 2^(N' + 2): 2M + 1 words
        pw_halfprod<ND, DB, 2 * M + 1, SQR>(ad, bd, [&](int k, u32 w) {
            if (k < M) Zw[M + k] = __builtin_addc(Zw[M + k], w, c, &c);        // + psl high
            else if (k < 2 * M) Zw[k - M] = __builtin_subc(Zw[k - M], w, b, &b);   // - psh low
            else clo -= (int)w;   // psh's word M: straight into the low chain's carry
        });
        clo -= (int)b;
        chi += (int)c;
    }
    const int top = pw_kara_fold<M>(Zw, clo, chi);
#pragma unroll
    for (int j = 0; j < M; ++j) Z[j] = ((u64)Zw[2 * j + 1] << 32) | Zw[2 * j];
    T = top;   // in {-1, 0}: the schoolbook path's contract
}

// z = a b mod p' for canonical a (La, ta), b (Lb, tb); result limbs + top (value = L + T 2^N'),
// T in {-1, 0} from either path (the Karatsuba recombination folds its halves' small signed
// carries back into the words).
// park: where the Karatsuba path keeps the half sums (PwParkLds / PwParkReg)
template <int M, typename ZT, typename PK = PwParkReg<2 * M>>
__host__ __device__ __forceinline__ void pw_mulmod(ZT &&Z, int &T, const u64 (&La)[M], int ta, const u64 (&Lb)[M], int tb,
                                                   PK park = PK{})
{
    if (ta | tb) {   // 2^N' == -1: the product is 1, -b or -a  (cf. mul_fft.c:3250)
        if (ta && tb) {
#pragma unroll
            for (int j = 0; j < M; ++j) Z[j] = j == 0;
            T = 0;
            return;
        }
        // -v = ~v + 1 - 2^N'  ->  limbs ~v, +1 at limb 0, top -1
        i128 acc = 1;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            acc += (i128)(~(ta ? Lb[j] : La[j]));
            Z[j] = (u64)acc;
            acc >>= 64;
        }
        T = -1 + (int)(i64)acc;
        return;
    }
    if constexpr (pw_kara<M>()) {
        pw_kara_product<M, false>(Z, T, La, Lb, park);
        return;
    }
    // Full product over 29-bit digits: a column sums at most ND < 64 products < 2^58, so one
    // v_mad_u64_u32 per digit product with no carry tracking (pw_halfprod over the whole
    // operands).  The 4M product words are folded on the fly: Z = lo - hi (2^N' == -1), the low
    // 2M words stored, the high 2M subtracted from them in one borrow chain.
    constexpr int DB = 29, ND = (64 * M + DB - 1) / DB;
    u32 ad[ND], bd[ND];
    pw_digits<DB, ND>(ad, [&](int i) -> u32 { return i < 2 * M ? (u32)(La[i >> 1] >> (32 * (i & 1))) : 0u; });
    pw_digits<DB, ND>(bd, [&](int i) -> u32 { return i < 2 * M ? (u32)(Lb[i >> 1] >> (32 * (i & 1))) : 0u; });
    u32 bw = 0;
    pw_halfprod<ND, DB, 4 * M>(ad, bd, [&](int k, u32 w) {
        if (k < 2 * M) pw_zword_init(Z, k, w);
        else pw_zword_put(Z, k - 2 * M, __builtin_subc(pw_zword_get(Z, k - 2 * M), w, bw, &bw));
    });
    T = -(int)bw;   // value = Z + T 2^N', T in {-1, 0}
}

// exchange: thread t publishes its value as words (normalised first: pw_norm); its top and
// pending exponent are the caller's (pw_level)
template <int M, int LK>
__device__ __forceinline__ void pw_publish_words(const u64 (&L)[M], u32 *Xw, int t)
{
    constexpr int K = 1 << LK;
    // (an opaque copy of this address, to keep the second base register of the rows past the
    // 64 KiB ds offset reach from living across the levels, cut the l = 4096 spills 84 -> 68 B
    // per lane and slowed the kernel 40.0 -> 44.5 ms: profiles/r05/pw_lds_product_ab.txt)
    u32 *col = Xw + t;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        col[(2 * j) * K] = (u32)L[j];
        col[(2 * j + 1) * K] = (u32)(L[j] >> 32);
    }
    // rows 2M .. (pw_combine GRP)
    if constexpr (pw_group(K) >= 2) col[2 * M * K] = ~(u32)L[0];
    if constexpr (pw_group(K) == 4) {
        col[(2 * M + 1) * K] = ~(u32)(L[0] >> 32);
        col[(2 * M + 2) * K] = ~(u32)L[1];
    }
}

// One forward (DIF) or inverse (DIT) length-K cyclic transform with root 2^W2 over
// the values of the K threads of this workgroup.  P: this thread's pending exponent.
// a mod n for a < 4n, without a division (every exponent here is a sum of a few reduced terms)
__device__ __forceinline__ unsigned pw_mod(unsigned a, unsigned n)
{
    a = a >= 2 * n ? a - 2 * n : a;
    return a >= n ? a - n : a;
}

// an opaque copy of the thread index: values derived from it are recomputed where used
// instead of kept live across the transforms (cf. rp_launder)
__device__ __forceinline__ int pw_launder(int t)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));
#endif
    return t;
}

// Exchange ordering inside one wave: a wave's LDS instructions execute in issue order, so a
// level whose butterfly partners share a wave (h < 64) needs no workgroup barrier -- only a
// compiler fence that keeps this level's reads after its publish and before the next
// publish.  Levels with h >= 64 exchange across waves and keep both __syncthreads.
__device__ __forceinline__ void pw_wave_sync()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// the combine of a forward level j whose rotation E mod N' is one of the odd multiples of
// N' / 2^(j+1) and the same for the whole wave: a scalar switch to the compile-time rotation
// (pw_combine FIXE); anything else (never, by pw_transform's derivation) takes the general form
// (Eu = the wave's E mod N', an odd multiple (2I + 1) N' / 2^(J+1): I selects the copy; the last
// copy also takes any other value, which pw_transform's derivation rules out -- checked exactly
// for both kernel shapes by tests/test_pw_host.py's simulation of the pending exponents)
template <int M, int LK, int J, int I = 0>
__device__ __forceinline__ void pw_combine_fixed(u64 (&L)[M], int &T, int &S, int alpha, const u32 *Xw, int packed, int q,
                                                 unsigned E, unsigned Eu)
{
    constexpr unsigned NP = 64 * M;
    constexpr unsigned C = (2 * I + 1) * (NP >> (J + 1));
    if constexpr (I + 1 < (1 << J)) {
        if (Eu == C) {
            pw_combine<M, LK, pw_pd<M, LK>(), (int)C>(L, T, S, alpha, Xw, packed, q, E);
            return;
        }
        pw_combine_fixed<M, LK, J, I + 1>(L, T, S, alpha, Xw, packed, q, E, Eu);
    } else {
        pw_combine<M, LK, pw_pd<M, LK>(), (int)C>(L, T, S, alpha, Xw, packed, q, E);
    }
}

// one level jj of the transform.  FIXJ >= 0 (forward transforms, level jj = FIXJ): E mod N' is
// wave-uniform and one of 2^FIXJ compile-time values (level 0: exactly N'/2) -- pw_transform
// UNW (the inverse's last level, h = K/2): the un-weighting theta^-t 2^-lk folded in -- with F the
// exponent it applies after the level (pw_unweight_exp), r = alpha 2^F own + 2^(E + F) x_q: own is
// read back rotated from the words it has just published for its partner, so the separate publish +
// rotated read of the un-weighting is gone (pw_slot_product)
template <int M, int LK>
__device__ __forceinline__ unsigned pw_unweight_exp(unsigned Pz, unsigned W2, int t)
{
    constexpr unsigned NP = 64 * M, N2 = 2 * NP;
    // theta^-t 2^-lk: 2^-(t W2 / 2 + lk), for a half-integer t W2 / 2 (sqrt 2)^-1 = sqrt 2 / 2:
    // 2^(-floor(t W2 / 2) - 1 - lk + N'/4) (2^(N'/2) - 1) -- the (2^(N'/2) - 1) factor by the caller
    const bool halff = (W2 & 1) && (t & 1);
    const unsigned un = (((unsigned)t * W2) >> 1) + LK + (halff ? 1 : 0);   // < N' + lk + 1
    return pw_mod(Pz + N2 - un + (halff ? NP / 4 : 0), N2);
}

template <int M, int LK, int DIR, int FIXJ, bool UNW = false>
__device__ __forceinline__ void pw_level(u64 (&L)[M], int &T, int &S, unsigned &P, u32 *Xw, int *TT, unsigned W2, int t,
                                         int jj, bool unw = false)
{
    constexpr int K = 1 << LK, lk = LK;
    constexpr unsigned N2 = 128 * M;
    const int j = DIR == 0 ? jj : lk - 1 - jj;   // DIF level index (DIT runs them backwards)
    const int h = K >> (j + 1);
    const int q = t ^ h;
    const bool top = !(t & h);
    const int qt = t & ~h;                       // top index of the pair
    // (qt mod h) 2^j < K/2, times W2: below N' (= K W2 / 2): no reduction needed
    const unsigned tw = (unsigned)((qt & (h - 1)) << j) * W2;
    const bool cross = h >= 64;                  // partner in another wave
    unsigned Pq;
    int packed;
    if (pw_tight(K)) {
        // the partner's top / sign and exponent first (a shuffle, or through rows 0-1 before
        // the words overwrite them), then the words
        T = pw_norm<M>(L, T);
        const int own = 2 * T + S;
        if (cross) {
            Xw[t] = (u32)own;
            Xw[K + t] = P;
            __syncthreads();
            packed = (int)Xw[q];
            Pq = Xw[K + q];
            __syncthreads();
        } else {
            packed = __shfl_xor(own, h);
            Pq = (unsigned)__shfl_xor((int)P, h);
        }
        pw_publish_words<M, LK>(L, Xw, t);
        if (cross) __syncthreads(); else pw_wave_sync();
    } else {
        // top / sign and pending exponent in one word (pw_pack_tp)
        T = pw_norm<M>(L, T);
        // (the partner's word by a wave shuffle ahead of the publish in the in-wave levels, as the
        // tight form takes it, measured no faster than this round trip: C3 6.7105 against 6.7169 ms
        // at equal prefetch distance, profiles/r17/pw_chain_ab.txt)
        pw_publish_words<M, LK>(L, Xw, t);
        TT[t] = (int)((unsigned)(2 * T + S) << 12 | P);
        if (cross) __syncthreads(); else pw_wave_sync();
        const int tp = TT[q];
        Pq = (unsigned)tp & 4095u;
        packed = tp >> 12;
    }
    const int own_packed = 2 * T + S;   // (UNW) as published: T normalised by pw_norm
    unsigned E;
    if (DIR == 0) {
        // top: X_t + X_q = 2^P (x_t + 2^(Pq-P) x_q); bottom: (X_q - X_t) w^tw = 2^(P+tw) (2^(Pq-P) x_q - x_t)
        E = pw_mod(Pq + N2 - P, N2);
        if constexpr (FIXJ == 0) {
            pw_combine<M, LK, pw_pd<M, LK>(), 32 * M>(L, T, S, top ? 1 : -1, Xw, packed, q, E);
        } else if constexpr (FIXJ > 0) {
            constexpr unsigned NP = 64 * M;
            const unsigned Em = E >= NP ? E - NP : E;
            const unsigned Eu = (unsigned)__builtin_amdgcn_readfirstlane((int)Em);   // wave-uniform (above)
            pw_combine_fixed<M, LK, FIXJ>(L, T, S, top ? 1 : -1, Xw, packed, q, E, Eu);
        } else {
            pw_combine<M, LK, pw_pd<M, LK>(), -1, pw_group(K)>(L, T, S, top ? 1 : -1, Xw, packed, q, E);
        }
        if (!top) P = pw_mod(P + tw, N2);
    } else {
        // top: Z_t + Z_q w^-tw = 2^P (z_t + 2^(Pq-tw-P) z_q)
        // bottom: Z_q - Z_t w^-tw = 2^(P-tw) (2^(Pq-P+tw) z_q - z_t)
        E = top ? pw_mod(Pq + 2 * N2 - tw - P, N2) : pw_mod(Pq + N2 - P + tw, N2);
        if (UNW && unw) {
            if (!top) P = pw_mod(P + N2 - tw, N2);
            const unsigned F = pw_unweight_exp<M, LK>(P, W2, pw_tight(K) ? pw_launder(t) : t);
            constexpr unsigned NP = 64 * M;
            const unsigned Eq = pw_mod(E + F, N2);
            pw_combine<M, LK, pw_pd<M, LK>(), -1, pw_group(K)>(L, T, S, 0, Xw, own_packed, t, top ? F : pw_mod(F + NP, N2));
            __builtin_amdgcn_sched_barrier(0);   // the two rotated reads one after the other
            pw_combine<M, LK, pw_pd<M, LK>(), -1, pw_group(K)>(L, T, S, 1, Xw, packed, q, Eq);
            P = 0;
        } else {
            pw_combine<M, LK, pw_pd<M, LK>(), -1, pw_group(K)>(L, T, S, top ? 1 : -1, Xw, packed, q, E);
            if (!top) P = pw_mod(P + N2 - tw, N2);
        }
    }
    if (cross) __syncthreads(); else pw_wave_sync();
}

// the highest compile-time-rotation level of operand B's transform in the late-B (l = 4096) form:
// level 0 only -- while B transforms, A's transformed limbs are live, and the switch copies of
// levels 1 and 2 pushed the kernel into spilling (96 -> 40 B per lane; C4 pointwise 34.0 -> 32.3 ms,
// levels 0-1: 32.6; profiles/r05/pw_fixb_ab.txt); operand B loaded with A (l <= 2048): levels 0-2
constexpr int pw_fixb_late = 0, pw_fixb_early = 2;
template <int M, int LK, int DIR, int FIXMAX = 2>
__device__ __forceinline__ void pw_transform(u64 (&L)[M], int &T, int &S, unsigned &P, u32 *Xw, int *TT, unsigned W2, int t)
{
    int jj = 0;
    if (DIR == 0) {
        // The forward levels' rotations at the top of the DIF.  Before level j, P_t is the weight
        // floor(t W2 / 2) (+ N'/4 for a half exponent: equal for t and its partner q = t ^ h_j) plus,
        // for every earlier level j' whose bit h_j' = K >> (j'+1) t has, the twiddle
        // ((t mod h_j') << j') W2.  q differs from t in bit h_j only, so
        //   E = Pq - P = +-[h_j W2 / 2 + sum_(j' < j, bit h_j' of t) (h_j << j') W2]
        //     = +-[N' / 2^(j+1) + sum N' / 2^(j - j')]   (K W2 = 2 N'),
        // an odd multiple of N' / 2^(j+1), fixed by the bits h_0 .. h_(j-1) of t and the sign by
        // bit h_j: wave-uniform while h_j >= 64.  Level 0: exactly N'/2 for every thread; levels
        // 1 .. log2(K/128): one of 2^j values, a scalar switch to the compile-time rotation (the
        // per-word wrap tests, addresses and complement masks fold away).  Each level is its own
        // inlined copy (peeled off the loop: one loop body with both forms spilled 3x more).
        static_assert(LK >= 7, "level 0's partner K/2 >= 64 lanes away");
        pw_level<M, LK, DIR, 0>(L, T, S, P, Xw, TT, W2, t, 0);
        if constexpr (LK >= 8 && FIXMAX >= 1) pw_level<M, LK, DIR, 1>(L, T, S, P, Xw, TT, W2, t, 1);   // h = K/4 >= 64
        if constexpr (LK >= 9 && FIXMAX >= 2) pw_level<M, LK, DIR, 2>(L, T, S, P, Xw, TT, W2, t, 2);   // h = K/8 >= 64
        jj = LK >= 9 && FIXMAX >= 2 ? 3 : LK >= 8 && FIXMAX >= 1 ? 2 : 1;
    }
    for (; jj < LK; ++jj) pw_level<M, LK, DIR, -1, DIR == 1>(L, T, S, P, Xw, TT, W2, t, jj, jj == LK - 1);
}

// Piece t of a coefficient in the reduced HBM form (coeff.hpp: limbs + carry masks +
// carry limb): limbs [t LP, t LP + LP) plus the carries into them -- the carry out of
// limb m lands in limb m + 1, the carry into limb 0 is minus the carry out of limb l-1
// and minus the carry limb (both weigh 2^N == -1); the carry out of the piece's top limb
// is the next piece's.  The value v (-2 <= v < 2^(64 LP) + 2^(64 LP - 64)) is returned as
// L + T 2^N', T in {-1, 0}: the convolution tolerates such pieces (|c_t| < K 2^(2B+1)
// still fits the headroom N' >= 2B + lk + 4, pdispatch.hpp), so the pointwise inputs need no
// canonicalisation pass.  A piece lies inside one 64-limb mask row (LP | 64).
// The loads of a piece (its LP limbs, its own carry-mask words and those of the limb below
// it, the slot's carry limb), issued before any of them is used (pw_piece_fetch), then the
// arithmetic (pw_piece_make): a workgroup requests all its pieces' bytes at once and waits
// one HBM round trip, where a load-compute-load order waited one per piece (the masks of
// the limb below depend on nothing loaded, so nothing forces the order).
template <int LP>
struct PwRaw {
    u64 v[LP];
    u64 pw, nw;     // carry masks of the piece's 64-limb row
    u64 pwp, nwp;   // of the row holding limb m0 - 1 (or l - 1 for piece 0)
    int top;
};

template <int LP>
__device__ __forceinline__ void pw_piece_fetch(PwRaw<LP> &R, const u64 *dig, const u64 *cbp, const int *topp, int l,
                                               int t)
{
    typedef unsigned long long pw_v2u __attribute__((ext_vector_type(2)));
    static_assert(LP % 2 == 0, "pieces of whole limb pairs");
    const int m0 = t * LP, W = m0 >> 6, mb = m0 ? m0 - 1 : l - 1, Wp = mb >> 6;
    // the piece's LP limbs as 16-byte loads (m0 even, slots 64-byte aligned)
#pragma unroll
    for (int j = 0; j < LP; j += 2) {
        const pw_v2u q = *(const pw_v2u *)(dig + m0 + j);
        R.v[j] = q.x;
        R.v[j + 1] = q.y;
    }
    const pw_v2u c = *(const pw_v2u *)(cbp + 2 * W), cp = *(const pw_v2u *)(cbp + 2 * Wp);
    R.pw = c.x;
    R.nw = c.y;
    R.pwp = cp.x;
    R.nwp = cp.y;
    R.top = *topp;
}

// the piece's value from its loaded bytes (above)
template <int M, int LP>
__device__ __forceinline__ void pw_piece_make(u64 (&L)[M], int &T, const PwRaw<LP> &R, int l, int t)
{
    const int m0 = t * LP, b0 = m0 & 63;
    const int mb = m0 ? m0 - 1 : l - 1, bp = mb & 63;
    const int kb = (int)((R.pwp >> bp) & 1) - (int)((R.nwp >> bp) & 1);
    const int cin = m0 ? kb : -kb - R.top;
    i64 c = cin;   // signed carry into the next limb
#pragma unroll
    for (int j = 0; j < LP; ++j) {
        const u64 v = R.v[j];
        const int k = j ? (int)((R.pw >> (b0 + j - 1)) & 1) - (int)((R.nw >> (b0 + j - 1)) & 1) : 0;
        const i64 add = c + k;        // |add| <= 4
        const u64 r = v + (u64)add;
        c = add >= 0 ? (i64)(r < v) : -(i64)(r > v);
        L[j] = r;
    }
    // the carry c out of limb LP - 1 in {-1, 0, 1}: limb LP = c, sign-extended above (one
    // register for all the upper limbs), top -1 for a negative piece
    const u64 up = c < 0 ? ~0ull : 0ull;
#pragma unroll
    for (int j = LP; j < M; ++j) L[j] = j == LP ? (c > 0 ? 1ull : up) : up;
    T = c < 0 ? -1 : 0;
}

template <int M, int LP>
__device__ __forceinline__ void pw_load_piece(u64 (&L)[M], int &T, const u64 *dig, const u64 *cbp, const int *topp,
                                              int l, int t)
{
    PwRaw<LP> R;
    pw_piece_fetch<LP>(R, dig, cbp, topp, l, t);
    pw_piece_make<M, LP>(L, T, R, l, t);
}

// limbs per piece of the instantiated k_pwss shapes: l / K (l = 1024: M = 10, LP = 4;
// l = 2048, 4096: M = 18, 20, LP = 8)
template <int M, int LK>
__host__ __device__ constexpr int pw_piece_limbs() { return M <= 12 ? 4 : 8; }

// Piece t of x0 + x1 (sub = 0) or x0 - x1 (sub = 1) for two reduced-form coefficients: the
// last DIF level of the row transform (h = 1, twiddle 1) applied piecewise -- linear, so the
// pieces of the sum / difference are the sums / differences of the pieces (|c_t| at most
// doubles: the headroom N' >= 2B + lk + 4 covers it, pdispatch.hpp).  Each piece is LP limbs plus a carry
// in {-1, 0, 1} (pw_load_piece); the LP + 1 limb result is sign-extended to M limbs, T = -1
// for a negative value.
template <int M, int LP>
__device__ __forceinline__ void pw_load_pair_bfly(u64 (&L)[M], int &T, const u64 *dig, const u64 *cb, const int *top,
                                                  long s0, int l, int cbw, int t, bool sub)
{
    u64 A[M], B[M];
    int Ta, Tb;
    {
        PwRaw<LP> RA, RB;   // both slots' bytes requested before either is used
        pw_piece_fetch<LP>(RA, dig + (size_t)s0 * l, cb + (size_t)s0 * cbw, top + s0, l, t);
        pw_piece_fetch<LP>(RB, dig + (size_t)(s0 + 1) * l, cb + (size_t)(s0 + 1) * cbw, top + s0 + 1, l, t);
        pw_piece_make<M, LP>(A, Ta, RA, l, t);
        pw_piece_make<M, LP>(B, Tb, RB, l, t);
    }
    // limbs LP .. M-1 of A, B are the sign extension (carry limb LP, then 0 / ~0): add LP + 1 limbs
    const u32 m = sub ? ~0u : 0u;
    u32 c = sub ? 1u : 0u;
#pragma unroll
    for (int j = 0; j <= LP; ++j) {
        const u32 lo = __builtin_addc((u32)A[j], (u32)B[j] ^ m, c, &c);
        const u32 hi = __builtin_addc((u32)(A[j] >> 32), (u32)(B[j] >> 32) ^ m, c, &c);
        L[j] = ((u64)hi << 32) | lo;
    }
    // the values are below 2^(64 LP + 2) in magnitude: limb LP's sign is the result's sign
    const u64 up = (i64)L[LP] < 0 ? ~0ull : 0ull;
#pragma unroll
    for (int j = LP + 1; j < M; ++j) L[j] = up;
    T = (i64)L[LP] < 0 ? -1 : 0;
    (void)Ta;
    (void)Tb;
}

// Piece t of output pos (0..3) of the row DIF's last two levels on the slot quad x0..x3
// (positions 4i..4i+3 of a row, the levels h = 2 and h = 1 of a length-NC DIF with root
// 2^(w NR)): z0 = (x0 + x2) + (x1 + x3), z1 = (x0 + x2) - (x1 + x3), z2 = (x0 - x2) + w (x1 - x3),
// z3 = (x0 - x2) - w (x1 - x3), with w = 2^(w NR NC / 4) = 2^(N/2): piece t of 2^(N/2) v is
// piece t ^ K/2 of v, negated for t < K/2 (2^N == -1) -- a load address, not arithmetic.
// Linear, so the pieces of z are signed sums of the inputs' pieces (|c_t| grows 4x: the inner
// ring's headroom covers it, pdispatch.hpp).  Sums are kept in LP + 1 limbs two's complement,
// one input piece formed at a time (registers), then sign-extended to M limbs.
template <int M, int LP, int K, int INFL = 2>
__device__ __forceinline__ void pw_load_quad_bfly(u64 (&L)[M], int &T, const u64 *dig, const u64 *cb, const int *top,
                                                  long s0, int pos, int l, int cbw, int t)
{
    u64 acc[LP + 1];
#pragma unroll
    for (int j = 0; j <= LP; ++j) acc[j] = 0;
    const int tr = t ^ (K / 2), sg = t >= K / 2 ? 1 : -1;
    // sign of input slot q in output pos; x1, x3 come from the rotated piece for pos >= 2
    auto sign_of = [&](int q) {
        return q == 0 ? 1 : q == 2 ? (pos < 2 ? 1 : -1)
             : (pos < 2 ? (pos == 0 ? 1 : -1) : (pos == 2 ? sg : -sg) * (q == 1 ? 1 : -1));
    };
    auto add = [&](const PwRaw<LP> &R, int q, int pt) {
        u64 X[M];
        int Tx;
        pw_piece_make<M, LP>(X, Tx, R, l, pt);
        // acc += sign * (limbs 0 .. LP of X): limb LP of X is the piece's carry, sign-extended
        const u32 m = sign_of(q) < 0 ? ~0u : 0u;
        u32 c = m & 1u;
#pragma unroll
        for (int j = 0; j <= LP; ++j) {
            const u32 lo = __builtin_addc((u32)acc[j], (u32)X[j] ^ m, c, &c);
            const u32 hi = __builtin_addc((u32)(acc[j] >> 32), (u32)(X[j] >> 32) ^ m, c, &c);
            acc[j] = ((u64)hi << 32) | lo;
        }
    };
    if (INFL == 1) {   // one input's bytes at a time (x0, x2, x1, x3)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = u < 2 ? 2 * u : 2 * (u - 2) + 1, pt = (q & 1) && pos >= 2 ? tr : t;
            PwRaw<LP> R;
            pw_piece_fetch<LP>(R, dig + (size_t)(s0 + q) * l, cb + (size_t)(s0 + q) * cbw, top + s0 + q, l, pt);
            add(R, q, pt);
        }
    } else
    // two inputs' bytes in flight at a time (x0, x2 at piece t; then x1, x3)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int qa = h, qb = h + 2, pt = h && pos >= 2 ? tr : t;
        PwRaw<LP> Ra, Rb;
        pw_piece_fetch<LP>(Ra, dig + (size_t)(s0 + qa) * l, cb + (size_t)(s0 + qa) * cbw, top + s0 + qa, l, pt);
        pw_piece_fetch<LP>(Rb, dig + (size_t)(s0 + qb) * l, cb + (size_t)(s0 + qb) * cbw, top + s0 + qb, l, pt);
        add(Ra, qa, pt);
        add(Rb, qb, pt);
    }
    // |sum| < 2^(64 LP + 3): limb LP's sign is the value's sign
    const u64 up = (i64)acc[LP] < 0 ? ~0ull : 0ull;
#pragma unroll
    for (int j = 0; j < M; ++j) L[j] = j <= LP ? acc[j] : up;
    T = (i64)acc[LP] < 0 ? -1 : 0;
}

// diagnostics (MPFFT_PW_STAMPS): thread 0 stamps phase boundary k of this workgroup
__device__ __forceinline__ void pw_stamp(unsigned long long *stamp, int t, int k)
{
    if (stamp && t == 0) stamp[k] = __builtin_amdgcn_s_memtime();
}

// omega = 2^W2, W2 = 2 N' / K (host: K / 2 divides N')
template <int M, int LK>
__host__ __device__ constexpr unsigned pw_w2()
{
    static_assert(((128u * M) >> LK) << LK == 128u * M, "omega must be a power of two");
    return (128u * M) >> LK;
}

// exponent of the negacyclic weight theta^t = 2^(t W2 / 2); a half-integer exponent (W2 and t odd)
// is 2^(floor(t W2 / 2) + N'/4) (2^(N'/2) - 1)  (sqrt 2 = 2^(N'/4) (2^(N'/2) - 1) in R'), the
// (2^(N'/2) - 1) by the caller (pw_sqrt2)
template <int M, int LK>
__device__ __forceinline__ unsigned pw_weight_exp(int t)
{
    constexpr unsigned NP = 64 * M, W2 = pw_w2<M, LK>();
    return (((unsigned)t * W2) >> 1) + (((W2 & 1) && (t & 1)) ? NP / 4 : 0);   // < N' + N'/4
}

// Cache record of one slot of a precomputed operand (k_pwsx writes it, k_pwsp reads it): the
// operand's pieces after the weight, the inner forward transform and pw_canon -- M rows of K
// limbs, limb j of thread t at [j K + t] (a wave's loads and stores are consecutive 8-byte
// words), then one meta word per thread: K (8 M + 4) bytes.
__host__ __device__ constexpr size_t pw_pre_slot_bytes(int M, int K) { return (size_t)K * (8 * (size_t)M + 4); }
static_assert(pw_pre_slot_bytes(10, 256) == 21504 && pw_pre_slot_bytes(18, 256) == 37888 &&
              pw_pre_slot_bytes(20, 512) == 83968, "the shipped shapes' records");
// the meta word: pw_canon's flag (the residue is 2^N', its limbs 0), the sign flag and the pending
// exponent P < 2 N' < 2^12
__host__ __device__ __forceinline__ u32 pw_pre_pack(int flag, int sign, unsigned P)
{
    return (u32)(flag & 1) << 13 | (u32)(sign & 1) << 12 | (P & 4095u);
}
__host__ __device__ __forceinline__ void pw_pre_unpack(u32 w, int &flag, int &sign, unsigned &P)
{
    flag = (int)(w >> 13) & 1;
    sign = (int)(w >> 12) & 1;
    P = w & 4095u;
}
static_assert(2 * 64 * 20 <= 4096, "pending exponents fit the meta word's 12 bits");

// The end of a slot's inner product or square, from the pointwise results 2^Pz (-1)^Sz (Z, Tz): the
// inverse transform with 2^-lk (division by K) and theta^-t, then the signed coefficients c_t into
// X (limb-major, M rows) and their signs (+ limb M) into TT; stamps 5 and 6, ends with a barrier
template <int M, int LK>
__device__ __forceinline__ void pw_slot_tail(u64 (&Z)[M], int Tz, int Sz, unsigned Pz, u64 *X, u32 *Xw, int *TT, int t,
                                             unsigned long long *stamp)
{
    constexpr int K = 1 << LK;
    constexpr unsigned W2 = pw_w2<M, LK>();
    pw_transform<M, LK, 1>(Z, Tz, Sz, Pz, Xw, TT, W2, t);
    pw_stamp(stamp, t, 5);
    // the rotation by theta^-t 2^-lk rode in the last level (pw_level UNW); the (2^(N'/2) - 1)
    // of a half-integer weight commutes with it (that level ended with a barrier: the u64 rows
    // below may cross columns)
    const int tf = pw_tight(K) ? pw_launder(t) : t;
    if ((W2 & 1) && (tf & 1)) pw_sqrt2<M>(Z, Tz);
    // signed coefficient c_t = v - s p', v in [0, 2^N'], s = (v > 2^(N'-1))
    const int zt = pw_canon<M>(Z, Tz);
    const int neg = zt || (Z[M - 1] >> 63);
    if (pw_tight(K)) {
        // as N'-bit two's complement: v - s (v - 1 = 2^N' - 1 for v = 2^N'), its top bit the sign
        u64 b = (u64)neg;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const u64 z = Z[j];
            X[j * K + t] = z - b;
            b = b && z == 0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j) X[j * K + t] = Z[j];
        TT[t] = neg | (zt << 1);                     // s, and limb M of v (2^N' only)
    }
    __syncthreads();
    pw_stamp(stamp, t, 6);
}

// inner product of one slot: forward transforms of the pieces (La, Ta), (Lb, Tb), the
// pointwise products in R', the inverse and the un-weighting; leaves the signed
// coefficients c_t in X (limb-major, M rows) and their signs (+ limb M) in TT (ends with a barrier)
// loadB(Lb, Tb): when given (the tight form), operand B's pieces are loaded only after A's
// forward transform, so the two operands' raw and formed pieces are never live together (the
// kernel's register peak at 128 VGPRs; B's load latency is hidden by the CU's other workgroup)
// PRE (k_pwsp): operand B is already weighted, transformed and canonical -- loadB(Lb, Tb) fetches
// its cache record, the limbs into Lb and the meta word (pw_pre_pack) into Tb, after A's forward
// transform and pw_canon; B's weight, transform and pw_canon are skipped
template <int M, int LK, bool PRE = false, typename LoadB = int>
__device__ __forceinline__ void pw_slot_product(u64 (&La)[M], int Ta, u64 (&Lb)[M], int Tb, u64 *X, u32 *Xw, int *TT,
                                                int t, unsigned long long *stamp, LoadB loadB = 0)
{
    constexpr bool late_b = !std::is_same<LoadB, int>::value;
    constexpr int K = 1 << LK;
    constexpr unsigned N2 = 128 * M, W2 = pw_w2<M, LK>();
    int Sa = 0, Sb = 0;                          // sign flags
    // negacyclic weight theta^t (pw_weight_exp).  Recomputed from an opaque copy of t where used
    // again at l = 4096 (pw_launder): kept live from here to the un-weighting they took VGPRs that
    // kernel spilled (144 -> 96 B per lane, C4 pointwise 35.8 -> 34.9 ms)
    const bool half = (W2 & 1) && (t & 1);
    unsigned Pa = pw_weight_exp<M, LK>(t), Pb = late_b || PRE ? 0u : Pa;
    if (half) {
        pw_sqrt2<M>(La, Ta);
        if (!late_b && !PRE) pw_sqrt2<M>(Lb, Tb);
    }
    pw_stamp(stamp, t, 1);
    pw_transform<M, LK, 0>(La, Ta, Sa, Pa, Xw, TT, W2, t);
    pw_stamp(stamp, t, 2);
    int cb = 0;
    if constexpr (!PRE) {
        if constexpr (late_b) {
            loadB(Lb, Tb);
            const int tb = pw_launder(t);
            Pb = pw_weight_exp<M, LK>(tb);
            if ((W2 & 1) && (tb & 1)) pw_sqrt2<M>(Lb, Tb);
        }
        pw_transform<M, LK, 0, late_b ? pw_fixb_late : pw_fixb_early>(Lb, Tb, Sb, Pb, Xw, TT, W2, t);
    }
    pw_stamp(stamp, t, 3);

    // ---- inner products: 2^Pa xa * 2^Pb xb = 2^(Pa + Pb) (xa xb) ---------------------
    const int ca = pw_canon<M, pw_canon_fast_a<PRE>(K)>(La, Ta);
    if constexpr (PRE) {
        // the record after A's pw_canon: its M limbs are not live across that (k_pwsp's register peak)
        static_assert(!PRE || late_b, "the cached form loads its record here");
        loadB(Lb, Tb);
        pw_pre_unpack((u32)Tb, cb, Sb, Pb);
        // the product's sign and exponent cross the digit products as one opaque word (as Sa, Sb,
        // Pa, Pb the l = 4096 forms spilled a register)
        Tb = pw_launder((int)pw_pre_pack(0, Sa ^ Sb, pw_mod(Pa + Pb, N2)));
    } else {
        cb = pw_canon<M, false>(Lb, Tb);
    }
    u64 Z[M];
    int Tz, Sz = Sa ^ Sb;
    if constexpr (pw_kara<M>()) {
        // Karatsuba: the half sums are parked in this thread's own LDS word column (the argument
        // below), the result's limbs stay in registers (half as many digits are live)
        pw_mulmod<M>(Z, Tz, La, ca, Lb, cb, PwParkLds{Xw + t, K});
    } else if (pw_tight(K)) {
        // the product's limbs through this thread's own LDS word column (B's transform ended
        // with an in-wave level: no other wave reads this column; the inverse's first publish
        // comes after): C4 pointwise 40.5 -> 40.0 ms, its spills 128 -> 84 B per lane; at
        // l = 2048 (no spills either way) the register form is faster (3.57 vs 3.67 ms),
        // profiles/r05/pw_lds_product_ab.txt
        pw_mulmod<M>(PwLdsZ{Xw + t, K}, Tz, La, ca, Lb, cb);
#pragma unroll
        for (int j = 0; j < M; ++j) Z[j] = ((u64)Xw[(2 * j + 1) * K + t] << 32) | Xw[2 * j * K + t];
    } else {
        pw_mulmod<M>(Z, Tz, La, ca, Lb, cb);
    }
    unsigned Pz = pw_mod(Pa + Pb, N2);
    if constexpr (PRE) pw_pre_unpack((u32)Tb, cb, Sz, Pz);   // (as packed above)
    pw_stamp(stamp, t, 4);

    pw_slot_tail<M, LK>(Z, Tz, Sz, Pz, X, Xw, TT, t, stamp);
}

// R = sum_t c_t 2^(B t) mod 2^N + 1 from X / TT, stored in the reduced HBM form at
// (pa, cbp, *topp).  c_t 2^(Bt) = v_t 2^(Bt) - s_t (2^(Bt) + 2^(N' + Bt)); positions >= N
// wrap negated.  Thread t of NTH sums output limbs m = t + NTH r (coalesced, consecutive
// per wave).  H (the l limb overflows) aliases X: written after a barrier.
// ACC (k_pwsa): the slot's previous value at (pa, cbp, *topp) is added: limb m of it, and the +-1
// carry out of limb m - 1 its mask words hold, enter limb m's sum; its top and the carry out of
// limb l - 1 weigh 2^N == -1 and enter limb 0 negated.  All of it is read in the summing loop, before
// the barriers in front of the first store, so the slot is updated in place; the output is the same
// reduced form.  (Requesting the old limbs ahead of the loop spilled 8 bytes at M = 18.)
template <int M, int LK, int NTH = (1 << LK), bool ACC = false>
__device__ __forceinline__ void pw_slot_output(const u64 *X, const int *TT, int *H, u64 *pa, u64 *cbp, int *topp, int l,
                                               int t)
{
    constexpr int K = 1 << LK;
    const int LP = l >> LK;                      // limbs per piece
    const int lane = t & 63;
    u64 fo[8];
    int ho[8];
    const int RPT = l / NTH;   // <= 8 (host)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        fo[r] = 0;
        ho[r] = 0;
        if (r >= RPT) continue;
        const int m = t + NTH * r;
        i128 S = 0;
        if constexpr (ACC) {
            const int q = m ? m - 1 : l - 1;
            const u64 pw = cbp[2 * (q >> 6)], nw = cbp[2 * (q >> 6) + 1];
            const int cin = (int)((pw >> (q & 63)) & 1) - (int)((nw >> (q & 63)) & 1);
            S = (i128)pa[m] + (m ? cin : -(cin + *topp));
        }
        // limb d of c_tp (0 .. M): two's complement in the tight form (limb M the sign extension)
        auto limb_of = [&](int d, int tp) -> i128 {
            i128 v;
            if (pw_tight(K)) {
                v = d < M ? (i128)X[(size_t)d * K + tp] : -(i128)(X[(size_t)(M - 1) * K + tp] >> 63);
            } else {
                const int tt = TT[tp];
                v = d < M ? (i128)X[(size_t)d * K + tp] : (i128)(tt >> 1);
                if ((tt & 1) && (d == 0 || d == M)) v -= 1;
            }
            return v;
        };
        // pieces whose limbs [t'LP, t'LP + M] cover m: t' = m / LP - j, j < M / LP + 1 -- a
        // fixed-trip loop of guarded reads (a runtime-bounded one serialised its LDS round trips)
        {
            constexpr int LPc = pw_piece_limbs<M, LK>(), KP = M / LPc + 1;
            const int hi = m / LPc;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const int tp = hi - j, d = m - tp * LPc;
                if (tp >= 0 && d <= M) S += limb_of(d, tp);
            }
        }
        // ... and through the wrap (limb m + l, negated): only m < M
        if (m < M) {
            const int mm = m + l;
            int lo = (mm - M + LP - 1) / LP;
            for (int tp = lo; tp <= K - 1; ++tp) S -= limb_of(mm - tp * LP, tp);
        }
        fo[r] = (u64)S;
        ho[r] = (int)(i64)(S >> 64);
    }
    __syncthreads();   // every X read done: H overwrites its first rows
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (r < RPT) H[t + NTH * r] = ho[r];
    __syncthreads();
    // limb m: f_m + hv_(m-1) -> limb + carry out in {-1, 0, 1} (reduced form; the top
    // limb's overflow wraps into limb 0 negated, and its carry weighs 2^N == -1)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r >= RPT) continue;
        const int m = t + NTH * r;
        const int hin = m ? H[m - 1] : -H[l - 1];
        const u64 f = fo[r];
        const u64 nf = f + (u64)(i64)hin;
        const int kout = hin >= 0 ? (int)(nf < f) : -(int)(nf > f);
        pa[m] = nf;
        const u64 pm = __ballot(kout == 1), nm = __ballot(kout == -1);
        if (lane == 0) {
            cbp[2 * (m >> 6)] = pm;
            cbp[2 * (m >> 6) + 1] = nm;
        }
    }
    if (t == 0) *topp = 0;
}

// LDS of a k_pwss / k_pwsq workgroup (pw_lds_bytes)
struct PwLds {
    u64 *X;     // M K limbs (2M word rows during the transforms)
    u32 *Xw;    // the same as words
    int *TT;    // K (none in the tight form), after the exchange rows
    int *H;     // l, over X (pw_slot_output)
};
template <int M, int LK>
__device__ __forceinline__ PwLds pw_lds_carve(unsigned char *smem)
{
    constexpr int K = 1 << LK;
    u32 *Xw = (u32 *)smem;
    return PwLds{(u64 *)smem, Xw, pw_tight(K) ? nullptr : (int *)(Xw + pw_row_words(M, K)), (int *)smem};
}

// The slot of block b of nb in the fused kernels, XCD-aware: workgroups are dealt round-robin to
// the 8 XCDs (blockIdx mod 8), each with its own L2.  FUSE 1: blocks b and b + 8 take the two slots
// of one pair, so the second reads of a pair's four inputs hit the same L2; FUSE 2: blocks b,
// b + 8, b + 16, b + 24 take the four slots of one quad.  Identity on the tail of < 16 / < 32 blocks.
template <int FUSE>
__device__ __forceinline__ long pw_fused_slot(long b, long nb)
{
    static_assert(FUSE == 1 || FUSE == 2, "slot pairs or quads");
    constexpr long G = 1 << FUSE;
    if (b >= nb - nb % (8 * G)) return b;
    const long x = b & 7, j = b >> 3;
    return G * (((j >> FUSE) << 3) + x) + (j & (G - 1));
}

// k_pwss<M, LK, FUSE>: A[slot] <- A[slot] * B[slot] mod 2^N + 1, one workgroup of K = 2^lk
// threads per slot; reduced-form inputs and output (HBM format of coeff.hpp).
// FUSE 1: the inputs are the slot pairs (2i, 2i+1) of a row *before* the last level of the
// forward row DIF (h = 1, twiddle 1); workgroup s forms the pieces of x0 + x1 (s even) or
// x0 - x1 (s odd) of both operands on load, so that level costs no HBM pass of its own
// (mul_fft.c:2392-2408's last FFT_radix2 level fused into the pointwise loop :3244-3253,
// cf. the reference's row/pointwise fusion IFFT_radix2_mfa_truncate_sqrt2_combined :2745).
// Both workgroups of a pair read all four inputs, so the product goes to C, not in place.
// FUSE 2: the last two levels on slot quads (pw_load_quad_bfly), the four workgroups of a quad
// on one XCD.
// (Fusing the inverse row DIT's first level as well needs both products in one workgroup:
// measured at 194-256 VGPRs, occupancy 2 -> 1, so the inverse side stays a pass.)
// The kernel's body is pw_mul_slot, shared with the accumulating k_pwsa below.

// the slot's output at `slot` of the arrays (dig, cb, top); ACC: added to what is there
template <int M, int LK, bool ACC>
__device__ __forceinline__ void pw_slot_store(const u64 *X, const int *TT, int *H, u64 *dig, u64 *cb, int *top, long slot,
                                              int l, int cbw, int t)
{
    pw_slot_output<M, LK, (1 << LK), ACC>(X, TT, H, dig + (size_t)slot * l, cb + (size_t)slot * cbw, top + slot, l, t);
}

// the workgroup of k_pwss (ACC false) and of k_pwsa (ACC true: the product is added to C[slot], at every FUSE)
template <int M, int LK, int FUSE, bool ACC>
__device__ __forceinline__ void pw_mul_slot(u64 *digA, u64 *cbA, int *topA, const u64 *digB, const u64 *cbB,
                                            const int *topB, int l, u64 *digC, u64 *cbC, int *topC,
                                            unsigned long long *dbg)
{
    // diagnostics (MPFFT_PW_STAMPS): thread 0 stamps the phase boundaries of this workgroup
    unsigned long long *stamp = dbg ? dbg + 8 * (size_t)blockIdx.x : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memtime();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = 1 << LK;
    const int t = threadIdx.x;
    const auto [X, Xw, TT, H] = pw_lds_carve<M, LK>(smem);
    const int cbw = cb_words(l);
    constexpr int CLP = pw_piece_limbs<M, LK>();   // == l / K (host: pw_inner_limbs)
    u64 La[M], Lb[M];
    int Ta = 0, Tb = 0;
    if (FUSE == 0 && pw_late_b(K)) {
        const long slot = blockIdx.x;
        pw_load_piece<M, CLP>(La, Ta, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
        auto loadB = [&](u64 (&L)[M], int &T) {
            pw_load_piece<M, CLP>(L, T, digB + (size_t)slot * l, cbB + (size_t)slot * cbw, topB + slot, l, t);
        };
        pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp, loadB);
        // every piece of A was read before the first barrier of A's transform: the output may
        // overwrite A in place
        pw_slot_store<M, LK, ACC>(X, TT, H, ACC ? digC : digA, ACC ? cbC : cbA, ACC ? topC : topA, slot, l, cbw, t);
    } else if (FUSE == 0) {
        const long slot = blockIdx.x;
        {
            PwRaw<CLP> RA, RB;   // both operands' bytes requested before either is used
            pw_piece_fetch<CLP>(RA, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
            pw_piece_fetch<CLP>(RB, digB + (size_t)slot * l, cbB + (size_t)slot * cbw, topB + slot, l, t);
            pw_piece_make<M, CLP>(La, Ta, RA, l, t);
            pw_piece_make<M, CLP>(Lb, Tb, RB, l, t);
        }
        __syncthreads();   // every piece read before any output limb is written (in place on A)
        pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp);
        pw_slot_store<M, LK, ACC>(X, TT, H, ACC ? digC : digA, ACC ? cbC : cbA, ACC ? topC : topA, slot, l, cbw, t);
    } else if (FUSE == 2) {
        // the row DIF's last two levels on load, slot quads
        const long slot = pw_fused_slot<2>(blockIdx.x, gridDim.x);
        const long s0 = slot & ~3L;
        const int pos = (int)(slot & 3);
        pw_load_quad_bfly<M, CLP, K, pw_a_infl>(La, Ta, digA, cbA, topA, s0, pos, l, cbw, t);
        if (pw_late_b(K)) {
            // (an opaque copy of t: the piece offsets and mask bit positions of A's loader are not
            // kept live across A's transform for reuse here)
            auto loadB = [&](u64 (&L)[M], int &T) {
                pw_load_quad_bfly<M, CLP, K, pw_late_infl>(L, T, digB, cbB, topB, s0, pos, l, cbw, pw_launder(t));
            };
            pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp, loadB);
        } else {
            pw_load_quad_bfly<M, CLP, K>(Lb, Tb, digB, cbB, topB, s0, pos, l, cbw, t);
            pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp);
        }
        pw_slot_store<M, LK, ACC>(X, TT, H, digC, cbC, topC, slot, l, cbw, t);
    } else {
        const long slot = pw_fused_slot<1>(blockIdx.x, gridDim.x);
        pw_load_pair_bfly<M, CLP>(La, Ta, digA, cbA, topA, slot & ~1L, l, cbw, t, slot & 1);
        if (pw_late_b(K)) {
            auto loadB = [&](u64 (&L)[M], int &T) {
                pw_load_pair_bfly<M, CLP>(L, T, digB, cbB, topB, slot & ~1L, l, cbw, t, slot & 1);
            };
            pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp, loadB);
        } else {
            pw_load_pair_bfly<M, CLP>(Lb, Tb, digB, cbB, topB, slot & ~1L, l, cbw, t, slot & 1);
            pw_slot_product<M, LK>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp);
        }
        pw_slot_store<M, LK, ACC>(X, TT, H, digC, cbC, topC, slot, l, cbw, t);
    }
    if (stamp) {
        __syncthreads();
        if (threadIdx.x == 0) stamp[7] = __builtin_amdgcn_s_memtime();
    }
}

template <int M, int LK, int FUSE>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_wpe<M, LK>()))) void k_pwss(u64 *digA, u64 *cbA, int *topA, const u64 *digB, const u64 *cbB,
                                                  const int *topB, int l, u64 *digC, u64 *cbC, int *topC,
                                                  unsigned long long *dbg)
{
    pw_mul_slot<M, LK, FUSE, false>(digA, cbA, topA, digB, cbB, topB, l, digC, cbC, topC, dbg);
}

// k_pwsa<M, LK, FUSE>: C[slot] <- C[slot] + A[slot] * B[slot] mod 2^N + 1 (the sums of products,
// mpfft_dot_*): k_pwss with its loaders for that FUSE and the accumulating pw_slot_output.  A and B
// are only read, at FUSE 0 as well.
template <int M, int LK, int FUSE>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_wpe<M, LK>()))) void k_pwsa(const u64 *digA, const u64 *cbA, const int *topA, const u64 *digB, const u64 *cbB,
                                                  const int *topB, int l, u64 *digC, u64 *cbC, int *topC,
                                                  unsigned long long *dbg)
{
    pw_mul_slot<M, LK, FUSE, true>((u64 *)digA, (u64 *)cbA, (int *)topA, digB, cbB, topB, l, digC, cbC, topC, dbg);
}

// ---------------------------------------------------------------------------
// squaring: A[slot] <- A[slot]^2 (k_pwsq).  One operand, so one set of pieces, one forward
// transform and a digit product that forms every off-diagonal term once.
// ---------------------------------------------------------------------------

// z = a^2 mod p' for canonical a (La, ta); result limbs + top (value = L + T 2^N').
// One digit array: column c sums the products ad[i] ad[c - i], i < c - i, once and doubles the
// sum, plus ad[c/2]^2 for even c -- ND (ND + 1) / 2 digit products instead of pw_mulmod's ND^2.
// Counted with multiplicity a column still has at most ND products below 2^58: the bound of
// pw_mulmod's schoolbook, and the same lo - hi fold (the same limbs and top as pw_mulmod(a, a)).
// Where pw_kara<M>() it takes pw_mulmod's Karatsuba routine instead, as three half squares.
// park: as pw_mulmod's
template <int M, typename ZT, typename PK = PwParkReg<2 * M>>
__host__ __device__ __forceinline__ void pw_sqrmod(ZT &&Z, int &T, const u64 (&La)[M], int ta, PK park = PK{})
{
    if (ta) {   // 2^N' == -1: the square is 1
#pragma unroll
        for (int j = 0; j < M; ++j) Z[j] = j == 0;
        T = 0;
        return;
    }
    if constexpr (pw_kara<M>()) {   // three half squares; the same chains as pw_mulmod(a, a), so the same limbs
        pw_kara_product<M, true>(Z, T, La, La, park);
        return;
    }
    constexpr int DB = 29, ND = (64 * M + DB - 1) / DB;
    static_assert(ND < 64, "column sums must stay below 2^64");
    u32 ad[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int b0 = d * DB, li = b0 >> 6, sh = b0 & 63;
        u64 x = La[li] >> sh;
        if (sh + DB > 64 && li + 1 < M) x |= La[li + 1] << (64 - sh);
        ad[d] = (u32)(x & ((1u << DB) - 1));
    }
    u128 acc = 0;          // bits [pos, ...) of the square not yet emitted
    int pos = 0, k = 0;    // compile-time after unrolling
    i64 bw = 0;            // borrow of the lo - hi fold
#pragma clang loop unroll(full)
    for (int c = 0; c < 2 * ND - 1; ++c) {
        u64 off = 0;
        const int i0 = c < ND ? 0 : c - ND + 1;
#pragma clang loop unroll(full)
        for (int i = i0; 2 * i < c; ++i) off += (u64)ad[i] * ad[c - i];
        u64 col = 2 * off;
        if (!(c & 1)) col += (u64)ad[c / 2] * ad[c / 2];
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_sched_barrier(0);   // one column's products live at a time (VGPRs)
#endif
        acc += (u128)col << (DB * c - pos);
        const bool last = c == 2 * ND - 2;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (k < 2 * M && (last || DB * (c + 1) - pos >= 64)) {
                const u64 limb = (u64)acc;
                acc >>= 64;
                pos += 64;
                if (k < M) {
                    Z[k] = limb;
                } else {                       // fold: Z[k - M] -= limb (borrow chain)
                    const u64 z = Z[k - M];
                    const u64 d1 = z - limb;
                    i64 b1 = (i64)(d1 > z);
                    const u64 d2 = d1 + (u64)bw;   // bw <= 0
                    b1 += bw < 0 ? (i64)(d2 > d1) : 0;
                    Z[k - M] = d2;
                    bw = -b1;
                }
                ++k;
            }
        }
    }
    T = (int)bw;   // value = Z + T 2^N', T in {-1, 0}
}

// inner square of one slot: pw_slot_product with one operand -- the weight (and pw_sqrt2) once,
// one forward transform, one pw_canon, the squares in R', then the same inverse and un-weighting;
// leaves the signed coefficients c_t in X and their signs in TT (ends with a barrier).  The
// stamps keep pw_slot_product's numbering (2 and 3 coincide: there is no second transform).
template <int M, int LK>
__device__ __forceinline__ void pw_slot_square(u64 (&La)[M], int Ta, u64 *X, u32 *Xw, int *TT, int t,
                                               unsigned long long *stamp)
{
    constexpr int K = 1 << LK;
    constexpr unsigned N2 = 128 * M, W2 = pw_w2<M, LK>();
    int Sa = 0;
    unsigned Pa = pw_weight_exp<M, LK>(t);       // negacyclic weight theta^t
    if ((W2 & 1) && (t & 1)) pw_sqrt2<M>(La, Ta);
    pw_stamp(stamp, t, 1);
    pw_transform<M, LK, 0>(La, Ta, Sa, Pa, Xw, TT, W2, t);
    pw_stamp(stamp, t, 2);
    pw_stamp(stamp, t, 3);

    // ---- inner squares: (2^Pa xa)^2 = 2^(2 Pa) xa^2; the sign flag squares away -------
    const int ca = pw_canon<M>(La, Ta);
    u64 Z[M];
    int Tz, Sz = 0;
    if constexpr (pw_kara<M>()) {
        pw_sqrmod<M>(Z, Tz, La, ca, PwParkLds{Xw + t, K});   // as pw_slot_product's Karatsuba branch
    } else if (pw_tight(K)) {
        // through this thread's own LDS word column, as pw_slot_product (the forward transform
        // ended with an in-wave level; the inverse's first publish comes after)
        pw_sqrmod<M>(PwLdsZ{Xw + t, K}, Tz, La, ca);
#pragma unroll
        for (int j = 0; j < M; ++j) Z[j] = ((u64)Xw[(2 * j + 1) * K + t] << 32) | Xw[2 * j * K + t];
    } else {
        pw_sqrmod<M>(Z, Tz, La, ca);
    }
    unsigned Pz = pw_mod(2 * Pa, N2);
    pw_stamp(stamp, t, 4);

    pw_slot_tail<M, LK>(Z, Tz, Sz, Pz, X, Xw, TT, t, stamp);
}

// k_pwsq<M, LK, FUSE>: A[slot] <- A[slot]^2 mod 2^N + 1, one workgroup of K = 2^lk threads per
// slot: k_pwss without operand B (no second set of pieces, no second forward transform, no
// pw_late_b: that only keeps two operands' pieces from being live together).  FUSE 0 squares in
// place; FUSE 1 / 2 take the row DIF's last level(s) on load (slot pairs / quads in k_pwss's
// XCD-aware order) and write to C.
template <int M, int LK, int FUSE>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_wpe<M, LK>()))) void k_pwsq(u64 *digA, u64 *cbA, int *topA, int l, u64 *digC, u64 *cbC, int *topC,
                                                  unsigned long long *dbg)
{
    unsigned long long *stamp = dbg ? dbg + 8 * (size_t)blockIdx.x : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memtime();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = 1 << LK;
    const int t = threadIdx.x;
    const auto [X, Xw, TT, H] = pw_lds_carve<M, LK>(smem);
    const int cbw = cb_words(l);
    constexpr int CLP = pw_piece_limbs<M, LK>();
    u64 La[M];
    int Ta = 0;
    if (FUSE == 0) {
        const long slot = blockIdx.x;
        pw_load_piece<M, CLP>(La, Ta, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
        __syncthreads();   // every piece read before any output limb is written (in place on A)
        pw_slot_square<M, LK>(La, Ta, X, Xw, TT, t, stamp);
        pw_slot_output<M, LK>(X, TT, H, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
    } else if (FUSE == 2) {
        const long slot = pw_fused_slot<2>(blockIdx.x, gridDim.x);
        const long s0 = slot & ~3L;
        const int pos = (int)(slot & 3);
        pw_load_quad_bfly<M, CLP, K, pw_a_infl>(La, Ta, digA, cbA, topA, s0, pos, l, cbw, t);
        pw_slot_square<M, LK>(La, Ta, X, Xw, TT, t, stamp);
        pw_slot_output<M, LK>(X, TT, H, digC + (size_t)slot * l, cbC + (size_t)slot * cbw, topC + slot, l, t);
    } else {
        const long slot = pw_fused_slot<1>(blockIdx.x, gridDim.x);
        pw_load_pair_bfly<M, CLP>(La, Ta, digA, cbA, topA, slot & ~1L, l, cbw, t, slot & 1);
        pw_slot_square<M, LK>(La, Ta, X, Xw, TT, t, stamp);
        pw_slot_output<M, LK>(X, TT, H, digC + (size_t)slot * l, cbC + (size_t)slot * cbw, topC + slot, l, t);
    }
    if (stamp) {
        __syncthreads();
        if (threadIdx.x == 0) stamp[7] = __builtin_amdgcn_s_memtime();
    }
}

// ---------------------------------------------------------------------------
// multiplication by a precomputed operand: operand B's slots are cached after their inner forward
// transform (k_pwsx, once), and k_pwsp multiplies A's slots by the cached records -- k_pwss without
// B's loads from the row arrays, its weight, its forward transform and its pw_canon.
// ---------------------------------------------------------------------------

// the slot of block b: the plain order at FUSE 0, k_pwss's XCD-aware order in the fused forms
template <int FUSE>
__device__ __forceinline__ long pw_block_slot(long b, long nb)
{
    if constexpr (FUSE == 0) return b;
    else return pw_fused_slot<FUSE>(b, nb);
}

// thread t's part of slot `slot`'s cache record: its M limbs into L, returns its meta word
template <int M, int LK>
__device__ __forceinline__ u32 pw_pre_load(u64 (&L)[M], const unsigned char *pre, long slot, int t)
{
    constexpr int K = 1 << LK;
    // (row bases on the workgroup-uniform record address, the thread's index a 32-bit offset: one
    // address register per lane for all the rows)
    const u64 *rec = (const u64 *)(pre + (size_t)slot * pw_pre_slot_bytes(M, K));
#pragma unroll
    for (int j = 0; j < M; ++j) L[j] = (rec + j * K)[(unsigned)t];
    return ((const u32 *)(rec + M * K))[(unsigned)t];
}

// operand B's pieces (Lb, Tb) of one slot into its cache record: pw_slot_product's treatment of B
// -- the weight (and pw_sqrt2), one forward transform, pw_canon -- then the coalesced store
template <int M, int LK>
__device__ __forceinline__ void pw_slot_precomp(u64 (&Lb)[M], int Tb, u32 *Xw, int *TT, int t, unsigned char *pre,
                                                long slot, unsigned long long *stamp)
{
    constexpr int K = 1 << LK;
    constexpr unsigned W2 = pw_w2<M, LK>();
    int Sb = 0;
    unsigned Pb = pw_weight_exp<M, LK>(t);
    if ((W2 & 1) && (t & 1)) pw_sqrt2<M>(Lb, Tb);
    pw_stamp(stamp, t, 1);
    pw_transform<M, LK, 0>(Lb, Tb, Sb, Pb, Xw, TT, W2, t);
    pw_stamp(stamp, t, 2);
    const int cb = pw_canon<M, false>(Lb, Tb);
    u64 *rec = (u64 *)(pre + (size_t)slot * pw_pre_slot_bytes(M, K));
#pragma unroll
    for (int j = 0; j < M; ++j) rec[j * K + t] = Lb[j];
    ((u32 *)(rec + M * K))[t] = pw_pre_pack(cb, Sb, Pb);
    pw_stamp(stamp, t, 3);
}

// k_pwsx<M, LK, FUSE>: B[slot] -> cache record `slot`, one workgroup of K threads per slot, k_pwss's
// loaders for B (FUSE 1 / 2: the row DIF's last level(s) on load, paid here once) and its slot
// order; no product and no output stage.
template <int M, int LK, int FUSE>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_wpe<M, LK>()))) void k_pwsx(const u64 *digB, const u64 *cbB, const int *topB, int l, unsigned char *pre,
                                                  unsigned long long *dbg)
{
    unsigned long long *stamp = dbg ? dbg + 8 * (size_t)blockIdx.x : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memtime();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = 1 << LK;
    const int t = threadIdx.x;
    const auto [X, Xw, TT, H] = pw_lds_carve<M, LK>(smem);
    const int cbw = cb_words(l);
    constexpr int CLP = pw_piece_limbs<M, LK>();
    const long slot = pw_block_slot<FUSE>(blockIdx.x, gridDim.x);
    u64 Lb[M];
    int Tb = 0;
    if (FUSE == 0) pw_load_piece<M, CLP>(Lb, Tb, digB + (size_t)slot * l, cbB + (size_t)slot * cbw, topB + slot, l, t);
    else if (FUSE == 2) pw_load_quad_bfly<M, CLP, K, pw_a_infl>(Lb, Tb, digB, cbB, topB, slot & ~3L, (int)(slot & 3), l, cbw, t);
    else pw_load_pair_bfly<M, CLP>(Lb, Tb, digB, cbB, topB, slot & ~1L, l, cbw, t, slot & 1);
    pw_slot_precomp<M, LK>(Lb, Tb, Xw, TT, t, pre, slot, stamp);
    (void)X;
    (void)H;
    if (stamp) {
        __syncthreads();
        if (threadIdx.x == 0) stamp[7] = __builtin_amdgcn_s_memtime();
    }
}

// k_pwsp<M, LK, FUSE>: A[slot] * cached B[slot] mod 2^N + 1.  A as in k_pwss (its loaders, weight
// and forward transform), B's record from the cache -- with A's pieces, or in the tight form after
// A's transform, where k_pwss loads B -- then the same product, inverse and output: to A in place
// (FUSE 0) or to C (FUSE 1, 2).  The cache is only read.
template <int M, int LK, int FUSE>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_wpe<M, LK>()))) void k_pwsp(u64 *digA, u64 *cbA, int *topA, const unsigned char *pre, int l, u64 *digC, u64 *cbC,
                                                  int *topC, unsigned long long *dbg)
{
    unsigned long long *stamp = dbg ? dbg + 8 * (size_t)blockIdx.x : nullptr;
    if (stamp && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memtime();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = 1 << LK;
    const int t = threadIdx.x;
    const auto [X, Xw, TT, H] = pw_lds_carve<M, LK>(smem);
    const int cbw = cb_words(l);
    constexpr int CLP = pw_piece_limbs<M, LK>();
    const long slot = pw_block_slot<FUSE>(blockIdx.x, gridDim.x);
    u64 La[M], Lb[M];
    int Ta = 0, Tb = 0;
    if (FUSE == 0) pw_load_piece<M, CLP>(La, Ta, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
    else if (FUSE == 2) pw_load_quad_bfly<M, CLP, K, pw_a_infl>(La, Ta, digA, cbA, topA, slot & ~3L, (int)(slot & 3), l, cbw, t);
    else pw_load_pair_bfly<M, CLP>(La, Ta, digA, cbA, topA, slot & ~1L, l, cbw, t, slot & 1);
    // B's record is loaded after A's transform and pw_canon in every form, not only the tight one
    // (pw_slot_product PRE): all M limbs of a record are live, where the upper limbs of k_pwss's
    // raw pieces are one sign register, and held across A's transform or pw_canon they spilled
    // (80-120 B per lane).  A's transform has barriers: every piece of A is read before the
    // in-place output.
    auto loadB = [&](u64 (&L)[M], int &T) { T = (int)pw_pre_load<M, LK>(L, pre, slot, pw_launder(t)); };
    pw_slot_product<M, LK, true>(La, Ta, Lb, Tb, X, Xw, TT, t, stamp, loadB);
    if (FUSE == 0) pw_slot_output<M, LK>(X, TT, H, digA + (size_t)slot * l, cbA + (size_t)slot * cbw, topA + slot, l, t);
    else pw_slot_output<M, LK>(X, TT, H, digC + (size_t)slot * l, cbC + (size_t)slot * cbw, topC + slot, l, t);
    if (stamp) {
        __syncthreads();
        if (threadIdx.x == 0) stamp[7] = __builtin_amdgcn_s_memtime();
    }
}

// ---------------------------------------------------------------------------
// small matrix products (mpfft_matmul_*): every operand's slots are cached once as k_pwsx records,
// and k_pwmm forms one result entry's slot from kk pairs of records -- the kk inner products summed
// in the inner ring, then one inverse transform and one output stage.
// ---------------------------------------------------------------------------
constexpr int PW_MM_MAX = 4;   // terms of one sum (MPFFT_MM_MAX)

// acc <- acc + (-1)^neg (W + Tw 2^N'), acc = A + Ta 2^N': one 32-bit carry chain; a subtraction
// adds ~W + 1 = 2^N' - W, so its carry out counts one less
template <int M>
__host__ __device__ __forceinline__ void pw_mm_add(u64 (&A)[M], int &Ta, const u64 (&W)[M], int Tw, bool neg)
{
    const u32 m = neg ? ~0u : 0u;
    u32 c = neg ? 1u : 0u;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const u32 lo = __builtin_addc((u32)A[j], (u32)W[j] ^ m, c, &c);
        const u32 hi = __builtin_addc((u32)(A[j] >> 32), (u32)(W[j] >> 32) ^ m, c, &c);
        A[j] = ((u64)hi << 32) | lo;
    }
    Ta += (int)c + (neg ? -1 - Tw : Tw);
}

// waves per SIMD k_pwmm is compiled for: two records, the product and the accumulator are live
// across pw_mulmod (k_pwsp: one record less), which does not fit k_pwss's 128 VGPRs where the
// product's own LDS column (the Karatsuba park, the tight form's product words) leaves no room
// for the accumulator
template <int M, int LK>
__host__ __device__ constexpr int pw_mm_wpe()
{
    // M = 10 fits k_pwss's budget (96 VGPRs); M = 18: 155 VGPRs, three workgroups per CU; M = 20:
    // 162 VGPRs, one workgroup of eight waves per CU.  At k_pwss's 128 VGPRs the two larger sizes
    // spilled 156 and 124 bytes per lane
    return M == 10 ? pw_wpe<M, LK>() : M == 18 ? 3 : 2;
}

// k_pwmm<M, LK, ACC>: C[slot] <- (ACC: C[slot] +) sum_{i < kk} rec(ea_i)[slot] * rec(eb_i)[slot] mod 2^N + 1,
// one workgroup of K threads per slot.  caches: cache regions of `stride` bytes each, region e
// holding the k_pwsx records of one operand (pw_pre_slot_bytes per slot); ea, eb: the kk <= PW_MM_MAX
// region indices of the terms' factors, 8 bits each, term 0 lowest.  The records are only read.
// The pending exponent of a record is a function of the thread index alone (pw_transform: the
// weight and the twiddles of the levels whose bit t has; pw_canon leaves it), so every term's
// product carries the same 2^(Pa + Pb) and the sum needs no rotation: products are added with
// their signs Sa ^ Sb.  After kk signed additions of products with tops in {-1, 0} the
// accumulator's top lies in [-2 kk, 2 kk]; pw_norm's device form and pw_combine's T_q != -1
// branch take any such small top.
template <int M, int LK, bool ACC>
__global__ __launch_bounds__(1 << LK) __attribute__((amdgpu_waves_per_eu(pw_mm_wpe<M, LK>()))) void k_pwmm(const unsigned char *caches, unsigned long long stride, int kk, unsigned ea,
                                                  unsigned eb, int l, u64 *digC, u64 *cbC, int *topC)
{
    // a record's pieces are below 2^(B + 2) in magnitude behind the quad loaders (pdispatch.hpp: 2 B + lk + 6
    // for one product); PW_MM_MAX summed products take ceil(log2 PW_MM_MAX) = 2 bits more
    static_assert(PW_MM_MAX <= 4 && 64 * M >= 2 * 64 * pw_piece_limbs<M, LK>() + LK + 6 + 2,
                  "inner headroom for PW_MM_MAX summed products");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = 1 << LK;
    constexpr unsigned N2 = 128 * M;
    const int t = threadIdx.x;
    const auto [X, Xw, TT, H] = pw_lds_carve<M, LK>(smem);
    const int cbw = cb_words(l);
    const long slot = blockIdx.x;
    u64 Z[M];
#pragma unroll
    for (int j = 0; j < M; ++j) Z[j] = 0;
    int Tz = 0;
    unsigned Pz = 0;
#pragma unroll 1
    for (int i = 0; i < kk; ++i) {
        const unsigned char *ra = caches + (size_t)((ea >> (8 * i)) & 255u) * stride;
        const unsigned char *rb = caches + (size_t)((eb >> (8 * i)) & 255u) * stride;
        u64 La[M], Lb[M], W[M];
        const u32 ma = pw_pre_load<M, LK>(La, ra, slot, pw_launder(t));
        const u32 mb = pw_pre_load<M, LK>(Lb, rb, slot, pw_launder(t));
        int ca, cb, Sa, Sb, Tw;
        unsigned Pa, Pb;
        pw_pre_unpack(ma, ca, Sa, Pa);
        pw_pre_unpack(mb, cb, Sb, Pb);
        // the product's sign and exponent cross the digit products as one opaque word (k_pwsp)
        const int meta = pw_launder((int)pw_pre_pack(0, Sa ^ Sb, pw_mod(Pa + Pb, N2)));
        if constexpr (pw_kara<M>()) {
            pw_mulmod<M>(W, Tw, La, ca, Lb, cb, PwParkLds{Xw + t, K});
        } else if (pw_tight(K)) {
            pw_mulmod<M>(PwLdsZ{Xw + t, K}, Tw, La, ca, Lb, cb);
#pragma unroll
            for (int j = 0; j < M; ++j) W[j] = ((u64)Xw[(2 * j + 1) * K + t] << 32) | Xw[2 * j * K + t];
        } else {
            pw_mulmod<M>(W, Tw, La, ca, Lb, cb);
        }
        int cz, Sz;
        pw_pre_unpack((u32)meta, cz, Sz, Pz);
        pw_mm_add<M>(Z, Tz, W, Tw, Sz != 0);
    }
    pw_slot_tail<M, LK>(Z, Tz, 0, Pz, X, Xw, TT, t, nullptr);
    pw_slot_output<M, LK, K, ACC>(X, TT, H, digC + (size_t)slot * l, cbC + (size_t)slot * cbw, topC + slot, l, t);
}
