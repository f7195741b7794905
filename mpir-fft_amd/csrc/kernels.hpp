// kernels.hpp -- the HIP kernels of the MI355X new_mpn_mul path (gfx950).
//
// Kernel map (DESIGN.md "Kernels"; reference functions in SURVEY 8a):
//   k_pass<U,LOGG,DIR>  2^LOGG coefficients of one column or row in registers,
//                       LOGG radix-2 levels (DIF forward / DIT inverse) with
//                       carry-save digits, one carry resolution at the store.
//                       Covers FFT_split_bits (fused into the first column
//                       pass), FFT_radix2_truncate_twiddle / FFT_radix2_twiddle /
//                       FFT_radix2 / IFFT_radix2 / IFFT_radix2_twiddle
//                       (mul_fft.c:1179, :1397, :786, :1444, :1964) and the MFA
//                       twiddles (README:89; applied at the row pass).
//   k_pairop<U>         the element-wise steps of the truncated inverse
//                       (IFFT_radix2_truncate_twiddle :1733 and
//                       IFFT_radix2_truncate1_twiddle :1604).
//   k_pointwise<U>      new_mpn_mulmod_2expp1 (mul_fft.c:3119 -> MPIR
//                       mpn_mulmod_2expp1): negacyclic 32-bit digit convolution,
//                       one workgroup per product.
//   k_scale<U>          the 2^-(depth+1) scaling + normmod loop (mul_fft.c:3256-3260).
//   k_comb_sum / k_carry_blocks / k_carry_apply
//                       FFT_combine_bits (mul_fft.c:207) as limb-parallel
//                       shifted sums plus a device-wide carry-lookahead.
#pragma once
#include "coeff.hpp"

struct PassArgs {
    u64 *dig[2];
    u64 *cb[2];
    int *top[2];
    const u64 *src[2];   // non-null: load coefficients straight from the operand (fused split)
    long nsrc[2];
    long src_chunk;      // 0: src is the whole operand; else the rank's column slice (src_limb, sharded.py)
    u64 bits1;
    u64 N;               // bits
    int l;               // limbs
    int lbM, lvl0;       // log2 transform length; first level of this pass
    u64 rho;             // exponent (bits) of the transform's root at level 0
    long sub_stride, pos_stride;
    int nsub, pos_off;
    int pbb;             // blocked positions: pos = (blk << pbb) | within, slot += blk * pbs (pbb = 30: none)
    long pbs;
    int sub_off;         // global index of sub-array 0 (row for the twiddle, column for the split)
    long jNC;            // fused split: coefficient index j = (pos_off + pos) * jNC + sub_off + sub
    int zero_from;       // forward: positions >= zero_from are zero inputs (of every operand of the launch)
    int zero_op[2];      // fused split (k_rpass MODE 2): the same bound per operand (grid row), rp_zero_row
                         // of its own coefficient count where the host knows it, else zero_from
    int need;            // forward: only blocks starting below `need` are live
    int need_lo;         // forward: ... and ending above `need_lo` (a rank that needs only its own
                         // rows of the columns: replicated forward columns, mpfft_shard_stage 7)
    int tw_mode;         // 1: pre-multiply by 2^(tw_w*pos*revbin(sub)), 2: post-multiply by its inverse
    u64 tw_w;
    int tw_lbR;
    int canon;           // canonical store (pointwise inputs)
    int ngroups;         // groups per sub-array
    int nbuf;            // LDS staging buffers (1 or 2)
    u64 scale_e;         // wave kernels: nonzero = fused final scaling by 2^scale_e (canonical store)
    int ablate;          // timing experiments only (MPFFT_ABLATE): 1 = no levels/twiddles, 2 = also no normalisation
    unsigned *zp;        // non-null: clear zp[0, zn) (the combine's look-back flags) -- saves a fill launch
    long zn;
    unsigned long long *dbg;   // diagnostics only (MPFFT_BP_STAMPS): per-workgroup s_memtime phase stamps
    // Pending exponents carried from one k_rpass DIF pass to the next pass of the same
    // transform (rkernels.hpp; every Exec, the stage API and the sharded path included: a
    // transform's last level leaves no pending exponent, so every stage output is exact and
    // nothing is handed across a stage boundary):
    int pcarry;          // the inputs still owe the DIF pending exponents of levels [lvl0 - pcarry, lvl0)
    int pkeep;           // leave every pending exponent in the output (the next pass applies them)
    // the truncated inverse's FILL step folded into a block's last DIT pass (k_rpass DIR 1,
    // mode bit 2): positions p >= fill_lo also store 2^(p fill_rho) x_p at position p + fill_off
    int fill_lo, fill_off;
    u64 fill_rho;
    // ... and the half-adds that follow it (itft1_r while t <= h) collapsed in that store: the
    // distances fill_off/2, fill_off/4, .. down to fill_hmin (0: none) join the fill values of
    // positions p and p + d for fill_lo <= p < d in registers, and only the surviving rows are stored
    int fill_hmin;
    int grp0;            // k_rpass DIF: the first live group of a sub-array (the launch covers only the
                         // live groups, [grp0, grp0 + ngroups): no empty 1024-thread workgroups)
};

// Grid-stride clear of PassArgs::zp; called at the top of every pass kernel, before
// any barrier, so it cannot change the kernel's synchronisation.
__device__ inline void pass_clear_flags(const PassArgs &a)
{
    if (!a.zp) return;
    const long nt = (long)blockDim.x * blockDim.y * blockDim.z;
    const long nthr = (long)gridDim.x * gridDim.y * gridDim.z * nt;
    const long bid = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long t = bid * nt + ((long)threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x;
    for (long i = t; i < a.zn; i += nthr) a.zp[i] = 0u;
}

// LDS carve for the coefficient kernels:
//   [stage: rb * 2l i64][edge: norm_edge_ints int32][scan scratch: norm_scr_u64 u64]
struct Lds {
    i64 *stage;
    int *edge;
    u64 *scr;
};

__host__ __device__ inline size_t lds_bytes(int l, int rb, int G, int U, int nw)
{
    size_t st = (size_t)rb * 2 * l * sizeof(i64);
    size_t ed = ((size_t)norm_edge_ints(G, U, nw) * sizeof(int) + 15) / 16 * 16;
    return st + ed + (size_t)norm_scr_u64(G, U, nw) * sizeof(u64);
}

template <int U, int G>
__device__ __forceinline__ Lds lds_carve(unsigned char *smem, int l, int rb, int nw)
{
    Lds d;
    d.stage = (i64 *)smem;
    unsigned char *p = smem + (size_t)rb * 2 * l * sizeof(i64);
    d.edge = (int *)p;
    p += ((size_t)norm_edge_ints(G, U, nw) * sizeof(int) + 15) / 16 * 16;
    d.scr = (u64 *)p;
    return d;
}

// Multiply x[i] by 2^e(i) (mod p) for the i with rot(i) true, e(i) in [0, 2N) uniform.
// rb >= G: every coefficient owns stage slot i, one write/read round (2 barriers).
// rb <  G: one coefficient at a time (large coefficients; 2 barriers each).
template <int U, int G, typename EF>
__device__ __forceinline__ void rotate_all(const WG &c, i64 (&x)[G][2 * U], EF efn, u64 N, int l, i64 *stage,
                                           int rb)
{
    // U == 1 (l <= 256): all G slots always fit (host guarantees rb >= G); keep one code path
    if (U == 1 || rb >= G) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const u64 e = efn(i);
            if (e) {
                rot_write<U>(c, x[i], stage + (size_t)i * 2 * l, l);
                any = true;
            }
        }
        if (!any) return;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const u64 e = efn(i);
            if (e) rot_read<U>(c, x[i], stage + (size_t)i * 2 * l, make_rot(e, N), l);
        }
        __syncthreads();
    } else if (U != 1) {
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const u64 e = efn(i);
            if (!e) continue;
            rot_write<U>(c, x[i], stage, l);
            __syncthreads();
            rot_read<U>(c, x[i], stage, make_rot(e, N), l);
            __syncthreads();
        }
    }
}

// legacy form used by the small kernels (explicit exponent array)
template <int U, int G>
__device__ __forceinline__ void rotate_set(const WG &c, i64 (&x)[G][2 * U], const u64 (&ee)[G], u64 N, int l,
                                           i64 *stage, int rb)
{
    rotate_all<U, G>(c, x, [&](int i) { return ee[i]; }, N, l, stage, rb);
}

template <int U, int G>
__device__ __forceinline__ void normalize_store(const WG &c, const i64 (&x)[G][2 * U], const long (&slot)[G],
                                                const bool (&keep)[G], bool canon, const Coef &st, int l,
                                                const Lds &sm)
{
    u64 y[G][U];
    int tv[G], cy[G][U];
    wg_norm_multi<U, G>(c, x, y, tv, cy, l, canon, sm.edge, sm.scr);
#pragma unroll
    for (int i = 0; i < G; ++i)
        if (keep[i]) store_coeff<U>(c, y[i], cy[i], tv[i], st, slot[i], l);
}

// U == 1 kernels run with <= 256 threads (l <= 256 limbs): let them use up to 256 VGPRs
#define MPF_LB(U) ((U) == 1 ? 256 : 1024)

template <int U, int LOGG, int DIR>
__global__ __launch_bounds__(MPF_LB(U)) void k_pass(PassArgs a)
{
    pass_clear_flags(a);
    constexpr int G = 1 << LOGG;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int l = a.l;
    const Lds sm = lds_carve<U, G>(smem, l, a.nbuf, c.nw);
    const int op = blockIdx.y;
    Coef st;
    st.dig = a.dig[op];
    st.cb = a.cb[op];
    st.top = a.top[op];
    const int sub = (int)(blockIdx.x / a.ngroups);
    const int grp = (int)(a.grp0 + blockIdx.x % a.ngroups);
    const int lobits = a.lbM - a.lvl0 - LOGG;
    const int lo = grp & ((1 << lobits) - 1);
    const int hi = grp >> lobits;
    const int bstart = hi << (a.lbM - a.lvl0);
    if (DIR == 0 && (bstart >= a.need || bstart + (1 << (a.lbM - a.lvl0)) <= a.need_lo)) return;  // whole block past the truncation point / outside the rows needed
    const u64 N2 = 2 * a.N;
    // position of element i: pos0 + i * pstep
    const int pos0 = bstart | lo;
    const int pstep = 1 << lobits;
    const long sbase = (long)sub * a.sub_stride;
    auto slot_of = [&](int i) -> long {
        const int ps = a.pos_off + pos0 + i * pstep;
        return sbase + (long)(ps >> a.pbb) * a.pbs + (long)(ps & ((1 << a.pbb) - 1)) * a.pos_stride;
    };

    i64 x[G][2 * U];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (DIR == 0 && pos0 + i * pstep >= a.zero_from) zero_coeff<U>(x[i]);
        else if (a.src[op])
            load_split<U>(c, x[i], a.src[op], a.nsrc[op], SrcSlice{a.src_chunk, a.jNC, a.sub_off},
                          (long)(a.pos_off + pos0 + i * pstep) * a.jNC + a.sub_off + sub, a.bits1, l);
        else load_coeff<U>(c, x[i], st, slot_of(i), l);
    }

    // MFA twiddles: 2^(tw_w * (pos_off + pos) * revbin(row)), always < 2N
    const u64 rsub = a.tw_mode ? (u64)revbin_dev(a.sub_off + sub, a.tw_lbR) : 0;
    const u64 tw0 = a.tw_w * (u64)(a.pos_off + pos0) * rsub, twst = a.tw_w * (u64)pstep * rsub;
    if (a.tw_mode == 1)
        rotate_all<U, G>(c, x, [&](int i) { return tw0 + (u64)i * twst; }, a.N, l, sm.stage, a.nbuf);

#pragma unroll
    for (int li = 0; li < LOGG; ++li) {
        const int level = DIR == 0 ? a.lvl0 + li : a.lvl0 + LOGG - 1 - li;
        const int jb = DIR == 0 ? LOGG - 1 - li : li;   // window bit of the butterfly partner
        const int h = 1 << (a.lbM - level - 1);
        // twiddle of the pair whose upper element is i (bit jb clear):
        //   (pos_i mod h) * rho 2^level = e0 + (i mod 2^jb) * estep,  always < N
        const u64 unit = a.rho << level;
        const u64 e0 = (u64)(pos0 & (h - 1)) * unit;
        const u64 estep = (u64)pstep * unit;
        if (DIR == 0) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if ((i >> jb) & 1) continue;
                const int k = i | (1 << jb);
#pragma unroll
                for (int q = 0; q < 2 * U; ++q) {
                    const i64 s = x[i][q] + x[k][q], d = x[i][q] - x[k][q];
                    x[i][q] = s;
                    x[k][q] = d;
                }
            }
            rotate_all<U, G>(c, x, [&](int k) -> u64 {
                if (!((k >> jb) & 1)) return 0;
                return e0 + (u64)(k & ((1 << jb) - 1)) * estep; }, a.N, l, sm.stage, a.nbuf);
        } else {
            rotate_all<U, G>(c, x, [&](int k) -> u64 {
                if (!((k >> jb) & 1)) return 0;
                const u64 e = e0 + (u64)(k & ((1 << jb) - 1)) * estep;
                return e ? N2 - e : 0; }, a.N, l, sm.stage, a.nbuf);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if ((i >> jb) & 1) continue;
                const int k = i | (1 << jb);
#pragma unroll
                for (int q = 0; q < 2 * U; ++q) {
                    const i64 s = x[i][q] + x[k][q], d = x[i][q] - x[k][q];
                    x[i][q] = s;
                    x[k][q] = d;
                }
            }
        }
    }

    if (a.tw_mode == 2)
        rotate_all<U, G>(c, x, [&](int i) -> u64 {
            const u64 e = tw0 + (u64)i * twst;
            return e ? N2 - e : 0; }, a.N, l, sm.stage, a.nbuf);

    long slot[G];
    bool keep[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        slot[i] = slot_of(i);
        const int bs = (pos0 + i * pstep) & ~(pstep - 1);
        keep[i] = DIR == 1 || (bs < a.need && bs + pstep > a.need_lo);
    }
    normalize_store<U, G>(c, x, slot, keep, a.canon != 0, st, l, sm);
}

// --------------------------------------------------------------------------
// element-wise steps of the truncated inverse column transform
// --------------------------------------------------------------------------
enum { OP_DOUBLE = 0, OP_HALFADD = 1, OP_FILL = 2, OP_FIX = 3, OP_TWOXMY = 4, OP_IBFLY = 5 };

struct PairArgs {
    u64 *dig;
    u64 *cb;
    int *top;
    u64 N;
    int l;
    int op;
    long NC;      // slot stride between rows
    int ncol;
    int off, h, i0, cnt;
    u64 rho;      // e_i = i * rho (mod 2N)
    int nb, hb[3], xoff;   // k_rchain: TWOXMY partner offsets, the enclosing IBFLY's top rows
};

template <int U>
__global__ __launch_bounds__(1024) void k_pairop(PairArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int l = a.l;
    const Lds sm = lds_carve<U, 2>(smem, l, 2, c.nw);
    const int col = (int)(blockIdx.x % a.ncol);
    const int i = a.i0 + (int)(blockIdx.x / a.ncol);
    long slot[2];
    slot[0] = (long)(a.off + i) * a.NC + col;
    slot[1] = (long)(a.off + i + a.h) * a.NC + col;
    const u64 N2 = 2 * a.N;
    const u64 e = (u32)((u64)i * a.rho) % (u32)N2;
    i64 x[2][2 * U];
    u64 ee[2] = {0, 0};
    bool keep[2] = {true, false};
    Coef st;
    st.dig = a.dig;
    st.cb = a.cb;
    st.top = a.top;
    load_coeff<U>(c, x[0], st, slot[0], l);
    if (a.op != OP_DOUBLE && a.op != OP_FILL) load_coeff<U>(c, x[1], st, slot[1], l);
    else zero_coeff<U>(x[1]);
    switch (a.op) {
    case OP_DOUBLE:
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) x[0][q] *= 2;
        break;
    case OP_HALFADD:  // a = (a + b) / 2
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) x[0][q] += x[1][q];
        ee[0] = N2 - 1;
        rotate_set<U, 2>(c, x, ee, a.N, l, sm.stage, 2);
        break;
    case OP_FILL:     // b = 2^e a
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) x[1][q] = x[0][q];
        ee[1] = e;
        rotate_set<U, 2>(c, x, ee, a.N, l, sm.stage, 2);
        keep[0] = false;
        keep[1] = true;
        break;
    case OP_FIX:      // d = a - b; b = 2^e d; a = a + d
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) {
            const i64 d = x[0][q] - x[1][q];
            x[0][q] += d;
            x[1][q] = d;
        }
        ee[1] = e;
        rotate_set<U, 2>(c, x, ee, a.N, l, sm.stage, 2);
        keep[1] = true;
        break;
    case OP_TWOXMY:   // a = 2a - b
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) x[0][q] = 2 * x[0][q] - x[1][q];
        break;
    default:          // OP_IBFLY: t = 2^-e b; a, b = a + t, a - t
        ee[1] = e ? N2 - e : 0;
        rotate_set<U, 2>(c, x, ee, a.N, l, sm.stage, 2);
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) {
            const i64 s = x[0][q] + x[1][q], d = x[0][q] - x[1][q];
            x[0][q] = s;
            x[1][q] = d;
        }
        keep[1] = true;
        break;
    }
    normalize_store<U, 2>(c, x, slot, keep, false, st, l, sm);
}

// --------------------------------------------------------------------------
// the sqrt2 front end's top level (new_mpn_mul6, mul_fft.c:3573-3668): the 4n-point
// transform pairs slot k (first half) with slot 2n + k (second half) through the 4n-th
// root of unity z = sqrt2^w (z^2 = 2^w), sqrt2 = 2^(3N/4) - 2^(N/4) mod 2^N + 1.
//   S2_FWD   split coefficients k, k + 2n of the operand (fused FFT_split_bits), then
//            (a, b) -> (a + b, z^k (a - b))       FFT_radix2_mfa_truncate_sqrt2 :2232-2281
//   S2_FILL  second half slot u <- z^u * first half slot u for the rows past trunc2
//            (the inputs known to be zero upstream)  IFFT_radix2_mfa_truncate_sqrt2 :2682-2692
//   S2_IBFLY (a, b) -> (a + z^-k b, a - z^-k b) for k < trunc - 2n, else a <- 2a  :2698-2740
// --------------------------------------------------------------------------
enum { S2_FWD = 0, S2_FILL = 1, S2_IBFLY = 2 };

struct S2Args {
    u64 *dig[2];
    u64 *cb[2];
    int *top[2];
    const u64 *src[2];   // S2_FWD: the operands
    long nsrc[2];
    u64 bits1;
    u64 N;
    u64 w;
    int l;
    int op;
    long half;           // 2n: slot offset of the second half
    long k0;             // first k of the launch (S2_FILL: trunc2 NC)
    long tlo;            // S2_IBFLY: pairs k < tlo, doubling above; S2_FWD: 0 = second half unused
};

// x[1] <- z^m x[1] (x[2] scratch): m w even: 2^(m w / 2); odd: 2^((m w - 1)/2) sqrt2 (FFT_twiddle_sqrt2 :972)
// add (< 2N): a further factor 2^add in the same rotation (the negacyclic un-weight's scaling)
template <int U>
__device__ __forceinline__ void s2_root(const WG &c, i64 (&x)[3][2 * U], u64 m, u64 w, u64 N, int l, i64 *stage, int rb,
                                        u64 add = 0)
{
    const u64 N2 = 2 * N, mw = m * w;
    u64 ee[3] = {0, 0, 0};
    if (!(mw & 1)) {
        ee[1] = (mw / 2 + add) % N2;
        rotate_set<U, 3>(c, x, ee, N, l, stage, rb);
        return;
    }
    const u64 e = (mw - 1) / 2 + add;
#pragma unroll
    for (int q = 0; q < 2 * U; ++q) x[2][q] = x[1][q];
    ee[1] = (e + 3 * N / 4) % N2;
    ee[2] = (e + N / 4) % N2;
    rotate_set<U, 3>(c, x, ee, N, l, stage, rb);
#pragma unroll
    for (int q = 0; q < 2 * U; ++q) {
        x[1][q] -= x[2][q];
        x[2][q] = 0;
    }
}

__host__ __device__ constexpr int s2_rb(int U) { return U == 1 ? 3 : 1; }

template <int U>
__global__ __launch_bounds__(1024) void k_s2op(S2Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int l = a.l;
    constexpr int RB = s2_rb(U);
    const Lds sm = lds_carve<U, 3>(smem, l, RB, c.nw);
    const int op = blockIdx.y;
    Coef st;
    st.dig = a.dig[op];
    st.cb = a.cb[op];
    st.top = a.top[op];
    const long k = a.k0 + (long)blockIdx.x;
    long slot[3] = {k, a.half + k, k};
    bool keep[3] = {true, true, false};
    i64 x[3][2 * U];
    zero_coeff<U>(x[2]);
    if (a.op == S2_FWD) {
        const SrcSlice whole{0, 1, 0};
        load_split<U>(c, x[0], a.src[op], a.nsrc[op], whole, k, a.bits1, l);
        load_split<U>(c, x[1], a.src[op], a.nsrc[op], whole, a.half + k, a.bits1, l);
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) {
            const i64 s = x[0][q] + x[1][q], d = x[0][q] - x[1][q];
            x[0][q] = s;
            x[1][q] = d;
        }
        if (a.tlo) s2_root<U>(c, x, (u64)k, a.w, a.N, l, sm.stage, RB);
        else keep[1] = false;
    } else if (a.op == S2_FILL) {
        load_coeff<U>(c, x[0], st, slot[0], l);
#pragma unroll
        for (int q = 0; q < 2 * U; ++q) x[1][q] = x[0][q];
        s2_root<U>(c, x, (u64)k, a.w, a.N, l, sm.stage, RB);
        keep[0] = false;
    } else {
        load_coeff<U>(c, x[0], st, slot[0], l);
        if (k < a.tlo) {
            load_coeff<U>(c, x[1], st, slot[1], l);
            s2_root<U>(c, x, (u64)(2 * a.half - k), a.w, a.N, l, sm.stage, RB);   // z^-k = z^(4n-k)
#pragma unroll
            for (int q = 0; q < 2 * U; ++q) {
                const i64 s = x[0][q] + x[1][q], d = x[0][q] - x[1][q];
                x[0][q] = s;
                x[1][q] = d;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 2 * U; ++q) {
                x[0][q] *= 2;
                x[1][q] = 0;
            }
            keep[1] = false;
        }
    }
    normalize_store<U, 3>(c, x, slot, keep, false, st, l, sm);
}

// --------------------------------------------------------------------------
// scaling by 2^-(depth+1) and canonicalisation (mul_fft.c:3256-3260)
// --------------------------------------------------------------------------
template <int U>
__global__ __launch_bounds__(1024) void k_scale(u64 *dig, u64 *cb, int *top, int l, u64 N, u64 e)
{
    Coef st;
    st.dig = dig;
    st.cb = cb;
    st.top = top;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const Lds sm = lds_carve<U, 1>(smem, l, 1, c.nw);
    long slot[1] = {(long)blockIdx.x};
    bool keep[1] = {true};
    i64 x[1][2 * U];
    u64 ee[1] = {e};
    load_coeff<U>(c, x[0], st, slot[0], l);
    rotate_set<U, 1>(c, x, ee, N, l, sm.stage, 1);
    normalize_store<U, 1>(c, x, slot, keep, true, st, l, sm);
}

// --------------------------------------------------------------------------
// pointwise products mod 2^N + 1 (one workgroup per slot), in place into A.
//   a b == sum_k Q_k X^k + S - a  (mod X^L + 1, X = 2^32), with
//   Q_k = sum_i a_i B'_{k-i+L},  B'_m = ~b_m (m < L), b_{m-L} (m >= L),
//   S = sum_i a_i.  Every column has exactly L unsigned terms (no divergence);
//   the complement trick turns the negacyclic wrap into the "- a + S" fix-up.
// LDS: A[L] u32, B'[2L] u32 (then reused as normalisation scratch).
// --------------------------------------------------------------------------
template <int U>
__global__ __launch_bounds__(1024) void k_pointwise(u64 *digA, u64 *cbA, int *topA, const u64 *digB,
                                                    const int *topB, int l, u64 N)
{
    Coef st;
    st.dig = digA;
    st.cb = cbA;
    st.top = topA;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int L = 2 * l;
    u32 *As = (u32 *)smem;
    u32 *Bs = As + L;
    u64 *scr = (u64 *)(smem + (size_t)3 * L * sizeof(u32));
    u64 *ssum = scr + norm_scr_u64(1, U, 16);
    const long slot = blockIdx.x;
    const int ta = topA[slot], tb = topB[slot];  // canonical inputs: tops in {0, 1}
    const u64 *pa = digA + (size_t)slot * l;
    const u64 *pb = digB + (size_t)slot * l;
    u64 asum = 0;
    if (c.t == 0) *ssum = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int m = u * c.nt + c.t;
        if (m < l) {
            const u64 va = pa[m], vb = pb[m];
            As[2 * m] = (u32)va;
            As[2 * m + 1] = (u32)(va >> 32);
            Bs[L + 2 * m] = (u32)vb;
            Bs[L + 2 * m + 1] = (u32)(vb >> 32);
            Bs[2 * m] = ~(u32)vb;
            Bs[2 * m + 1] = ~(u32)(vb >> 32);
            asum += (va & MPF_M32) + (va >> 32);
        }
    }
    __syncthreads();
    i64 d[2 * U];
    if (ta | tb) {
        // 2^N == -1: the product is -b, -a or 1 (MPIR's c flags, mul_fft.c:3250)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int m = u * c.nt + c.t;
            d[2 * u] = d[2 * u + 1] = 0;
            if (m < l) {
                if (ta && tb) {
                    d[2 * u] = (m == 0) ? 1 : 0;
                } else {
                    const u32 *o = ta ? (Bs + L) : As;
                    d[2 * u] = -(i64)o[2 * m];
                    d[2 * u + 1] = -(i64)o[2 * m + 1];
                }
            }
        }
        __syncthreads();
    } else {
        for (int off = 32; off > 0; off >>= 1) asum += __shfl_xor(asum, off);
        if (c.lane == 0) atomicAdd((unsigned long long *)ssum, (unsigned long long)asum);
        u64 r1[U];
        i64 q0[2 * U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int m = u * c.nt + c.t;
            q0[2 * u] = q0[2 * u + 1] = 0;
            r1[u] = 0;
            if (m < l) {
                const int k0 = 2 * m;
                u64 acc0 = 0, acc1 = 0;
                u32 h0 = 0, h1 = 0;
                const u32 *bp = Bs + k0 + L;
                for (int i = 0; i < L; ++i) {
                    const u64 av = As[i];
                    const u64 p0 = av * bp[-i];
                    const u64 p1 = av * bp[1 - i];
                    acc0 += p0;
                    h0 += (acc0 < p0);
                    acc1 += p1;
                    h1 += (acc1 < p1);
                }
                // Q_k = q0_k + r_k X with r_k = Q_k >> 32 (< 2^45)
                const u64 rk0 = (acc0 >> 32) | ((u64)h0 << 32);
                const u64 rk1 = (acc1 >> 32) | ((u64)h1 << 32);
                q0[2 * u] = (i64)(acc0 & MPF_M32) - (i64)As[k0];
                q0[2 * u + 1] = (i64)(acc1 & MPF_M32) - (i64)As[k0 + 1] + (i64)rk0;
                r1[u] = rk1;
            }
        }
        __syncthreads();
        i64 *sh = (i64 *)smem;  // As/Bs are dead now
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int m = u * c.nt + c.t;
            if (m < l) sh[m] = (i64)r1[u];
        }
        __syncthreads();
        const i64 S = (i64)*ssum;
        const i64 rl = sh[l - 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int m = u * c.nt + c.t;
            d[2 * u] = q0[2 * u];
            d[2 * u + 1] = q0[2 * u + 1];
            if (m < l) d[2 * u] += m ? sh[m - 1] : (S - rl);  // X^L == -1 wraps r_{L-1}
        }
        __syncthreads();
    }
    i64 dd[1][2 * U];
#pragma unroll
    for (int q = 0; q < 2 * U; ++q) dd[0][q] = d[q];
    long slots[1] = {slot};
    bool keep[1] = {true};
    Lds sm;
    sm.stage = nullptr;
    sm.edge = (int *)smem;                       // As/Bs are dead by now
    sm.scr = scr;
    normalize_store<U, 1>(c, dd, slots, keep, false, st, l, sm);  // reduced: the inverse pass folds the carries
}

// --------------------------------------------------------------------------
// k_pw<R>: the register-blocked pointwise product (even l).  Same algebra as
// k_pointwise; thread t owns the R consecutive columns [R t, R t + R) and walks
// the L terms 4 at a time: per step one broadcast ds_read_b128 of a[i..i+3], an
// aligned window of R+4 digits of B' (ds_read_b128, conflict-free across lanes),
// and 4R multiply-accumulates, each one v_mad_u64_u32 into a 64-bit accumulator
// whose carry-out feeds a 32-bit high word (v_addc) -- 2 VALU per 32x32 MAC.
// Columns are then handed to the normaliser's strided limb ownership through LDS.
// blockDim = L / R (>= 64), U = R / 2 limbs per thread in the normaliser.
// --------------------------------------------------------------------------
// four independent 32x32 -> 96-bit multiply-accumulates: acc_k += a * b_k, carry into h_k.
// Each v_mad_u64_u32 writes its own SGPR-pair carry, read by its v_addc three
// instructions later (gfx950 needs 2 wait states between a VALU SGPR write and a
// VALU read of it; the assembler inserts none inside inline asm).
__device__ __forceinline__ void mac4(u64 &a0, u64 &a1, u64 &a2, u64 &a3, u32 &h0, u32 &h1, u32 &h2, u32 &h3,
                                     u32 a, u32 b0, u32 b1, u32 b2, u32 b3)
{
    u64 c0, c1, c2, c3;
    asm("v_mad_u64_u32 %0, %8, %12, %13, %0\n\t"
        "v_mad_u64_u32 %1, %9, %12, %14, %1\n\t"
        "v_mad_u64_u32 %2, %10, %12, %15, %2\n\t"
        "v_mad_u64_u32 %3, %11, %12, %16, %3\n\t"
        "v_addc_co_u32_e64 %4, %8, 0, %4, %8\n\t"
        "v_addc_co_u32_e64 %5, %9, 0, %5, %9\n\t"
        "v_addc_co_u32_e64 %6, %10, 0, %6, %10\n\t"
        "v_addc_co_u32_e64 %7, %11, 0, %7, %11"
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3),
          "=&s"(c0), "=&s"(c1), "=&s"(c2), "=&s"(c3)
        : "v"(a), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
}

template <int R>
__global__ __launch_bounds__(1024) void k_pw(u64 *digA, u64 *cbA, int *topA, const u64 *digB, const int *topB,
                                             int l)
{
    constexpr int U = R / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int L = 2 * l;
    u32 *As = (u32 *)smem;            // L digits of a
    u32 *Bs = As + L;                 // B'[0, 2L)
    u64 *scr = (u64 *)(smem + (size_t)3 * L * sizeof(u32));
    u64 *ssum = scr + norm_scr_u64(1, U, 16);
    Coef st;
    st.dig = digA;
    st.cb = cbA;
    st.top = topA;
    const long slot = blockIdx.x;
    const int ta = topA[slot], tb = topB[slot];  // canonical inputs: tops in {0, 1}
    const u64 *pa = digA + (size_t)slot * l;
    const u64 *pb = digB + (size_t)slot * l;
    if (c.t == 0) *ssum = 0;
    // strided ownership (normaliser layout): limb m = u * nt + t
    u64 amine[U];
    u64 asum = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int m = u * c.nt + c.t;
        amine[u] = 0;
        if (m < l) {
            const u64 va = pa[m], vb = pb[m];
            amine[u] = va;
            As[2 * m] = (u32)va;
            As[2 * m + 1] = (u32)(va >> 32);
            Bs[L + 2 * m] = (u32)vb;
            Bs[L + 2 * m + 1] = (u32)(vb >> 32);
            Bs[2 * m] = ~(u32)vb;
            Bs[2 * m + 1] = ~(u32)(vb >> 32);
            asum += (va & MPF_M32) + (va >> 32);
        }
    }
    __syncthreads();
    i64 d[1][2 * U];
    if (ta | tb) {
        // 2^N == -1: the product is -b, -a or 1 (MPIR's c flags, mul_fft.c:3250)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            d[0][2 * u] = d[0][2 * u + 1] = 0;
            if (m < l) {
                if (ta && tb) {
                    d[0][2 * u] = (m == 0) ? 1 : 0;
                } else {
                    const u32 *o = ta ? (Bs + L) : As;
                    d[0][2 * u] = -(i64)o[2 * m];
                    d[0][2 * u + 1] = -(i64)o[2 * m + 1];
                }
            }
        }
        __syncthreads();
    } else {
        for (int off = 32; off > 0; off >>= 1) asum += __shfl_xor(asum, off);
        if (c.lane == 0) atomicAdd((unsigned long long *)ssum, (unsigned long long)asum);
        const int k0 = R * c.t;
        u64 acc[R];
        u32 hh[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r] = 0;
            hh[r] = 0;
        }
        if (k0 < L) {
            // window for term block i0: B'[k0 - i0 - 4 + L, +R+4), 16-byte aligned (k0, i0, L = 0 mod 4)
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            const v4u *bw = (const v4u *)(Bs + k0 - 4 + L);
            const v4u *a4p = (const v4u *)As;
            constexpr int NW = R / 4 + 1;
            v4u av = a4p[0];
            v4u bv[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                bv[k] = bw[k];
                asm volatile("" : "+v"(bv[k]));   // keep the whole 16-byte read (one ds_read_b128)
            }
            for (int i4 = 0; i4 < L / 4; ++i4) {
                // prefetch the next block while this one is multiplied
                const int nx = (i4 + 1 < L / 4) ? i4 + 1 : i4;
                const v4u avn = a4p[nx];
                v4u bvn[NW];
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    bvn[k] = bw[k - nx];
                    asm volatile("" : "+v"(bvn[k]));
                }
                u32 w[4 * NW];
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    w[4 * k] = bv[k].x; w[4 * k + 1] = bv[k].y; w[4 * k + 2] = bv[k].z; w[4 * k + 3] = bv[k].w;
                }
                const u32 a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int r = 0; r < R; r += 4)
                        mac4(acc[r], acc[r + 1], acc[r + 2], acc[r + 3], hh[r], hh[r + 1], hh[r + 2], hh[r + 3],
                             a4[q], w[4 + r - q], w[5 + r - q], w[6 + r - q], w[7 + r - q]);
                av = avn;
#pragma unroll
                for (int k = 0; k < NW; ++k) bv[k] = bvn[k];
            }
        }
        __syncthreads();  // As/Bs dead: reuse as q0buf[L] u32 + rbuf[L] u64
        u32 *q0b = (u32 *)smem;
        u64 *rb = (u64 *)(smem + (size_t)L * sizeof(u32));
        if (k0 < L) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                q0b[k0 + r] = (u32)acc[r];
                rb[k0 + r] = (acc[r] >> 32) | ((u64)hh[r] << 32);   // Q_k >> 32  (< 2^45)
            }
        }
        __syncthreads();
        const i64 S = (i64)*ssum;
        const i64 rl = (i64)rb[L - 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            d[0][2 * u] = d[0][2 * u + 1] = 0;
            if (m < l) {
                const int j = 2 * m;
                // a b == sum_k (q0_k + r_{k-1}) X^k + S - a, r_{-1} -> -r_{L-1}
                d[0][2 * u] = (i64)q0b[j] - (i64)(amine[u] & MPF_M32) + (j ? (i64)rb[j - 1] : S - rl);
                d[0][2 * u + 1] = (i64)q0b[j + 1] - (i64)(amine[u] >> 32) + (i64)rb[j];
            }
        }
        __syncthreads();
    }
    long slots[1] = {slot};
    bool keep[1] = {true};
    Lds sm;
    sm.stage = nullptr;
    sm.edge = (int *)smem;
    sm.scr = scr;
    normalize_store<U, 1>(c, d, slots, keep, false, st, l, sm);   // reduced: the inverse pass folds the carries
}

// --------------------------------------------------------------------------
// k_pwm<U,FT>: the pointwise product on the matrix cores (l % 128 == 0).
//
// A big-integer product is a Toeplitz matrix times a vector; split into 32-byte
// blocks it becomes a GEMM that v_mfma_i32_32x32x32_i8 runs at 32 K-terms per
// lane-pair per instruction.  With bytes u_i of a, v_j of b (L8 = 8 l of each):
//   c_m = sum_i u_i v_{m-i},   output block p holds c_{32p + s}, s < 32,
//   C[s][p] = sum_d sum_t Tq_d[s][t] * vb_{p-d}[t],  Tq_d[s][t] = u_{32d + s - t},
// i.e. for every block distance d one 32x32 Toeplitz tile of a (A operand) times
// a sliding window of 32 consecutive 32-byte blocks of b (B operand), accumulated
// over d in the MFMA accumulator.  The i8 MFMA is signed, so digits are offset
// binary: s_i = u_i - 128 (= byte ^ 0x80), t_j = v_j - 128, and
//   c_m = conv(s, t)_m + 128 W(m),  W(m) = sum_{i in win(m)} (u_i + v_i - 128)
// (win(m) = [max(0, m-L8+1), min(m, L8-1)]), a prefix-sum correction.
// Negacyclic fold (2^N == -1): output block p and p + NB (NB = l/4 blocks) land
// in the same lane and register of the two accumulators a wave keeps per "fold
// tile" (32 output blocks), so digit q (32-bit, X = 2^32) of the residue is
//   F_q = sum_e 2^(8e) (lo - hi)[row 4q+e] + 128 sum_e 2^(8e) (2 PZ[4q+e] - PZ_tot).
// |F_q| < 2^57 at l = 4096; the canonical normaliser takes |digit| < 2^62.
// MFMA operands: A lane (r, h) holds s_{32d + r - 16h - j}, j < 16 (16 bytes of
// the byte-reversed a at a lane-dependent byte offset: 5 aligned dword reads +
// v_alignbyte), B lane (c, h) holds t bytes [32(p - d) + 16h, +16) (one aligned
// ds_read_b128).  Element j of lane half h pairs A and B by the same t = 16h + j,
// so the hardware's own k order inside a fragment does not matter.
// C/D map (gfx950, dtype-independent): col = lane & 31, row = (reg & 3) + 8 (reg >> 2)
// + 4 (lane >> 5): each lane's 4 consecutive rows are the 4 bytes of one digit.
// Per slot: NB/32 fold tiles x (NB + 32) MFMAs; one workgroup per slot, wave w
// owns fold tiles w, w + nw, ...; blockDim = 64 min(NB/32, 16), U = l / blockDim.
// LDS: SR[L8 + 96] (reversed s, 32-byte zero pads) | TB[L8 + 2048] (t, 1 KB
// zero pads) | PZ[L32 + 1] int | wave sums | normaliser scratch; the digit
// array DG[L32] i64 reuses SR/TB after the MFMA phase.
// Reference: new_mpn_mulmod_2expp1 (mul_fft.c:3119) -> MPIR mpn_mulmod_2expp1.
// --------------------------------------------------------------------------
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));

__host__ __device__ inline size_t pwm_lds_bytes(int l, int U, int nw)
{
    const size_t L8 = 8 * (size_t)l;
    size_t b = (L8 + 96) + (L8 + 2048) + ((2 * (size_t)l + 1) * 4 + 15) / 16 * 16 + 64;
    b += ((size_t)norm_edge_ints(1, U, nw) * sizeof(int) + 15) / 16 * 16;
    return b + (size_t)norm_scr_u64(1, U, nw) * sizeof(u64);
}

template <int U, int FT>
__global__ __launch_bounds__(1024) void k_pwm(u64 *digA, u64 *cbA, int *topA, const u64 *digB, const int *topB,
                                              int l)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int L8 = 8 * l, NB = l / 4, L32 = 2 * l;
    unsigned char *SR = smem;
    unsigned char *TB = SR + L8 + 96;
    int *PZ = (int *)(TB + L8 + 2048);
    int *wsum = PZ + ((L32 + 1) * 4 + 15) / 16 * 4;
    Lds sm;
    sm.stage = nullptr;
    sm.edge = wsum + 16;
    sm.scr = (u64 *)((unsigned char *)sm.edge + ((size_t)norm_edge_ints(1, U, c.nw) * sizeof(int) + 15) / 16 * 16);
    Coef st;
    st.dig = digA;
    st.cb = cbA;
    st.top = topA;
    const long slot = blockIdx.x;
    const int ta = topA[slot], tb = topB[slot];  // canonical inputs: tops in {0, 1}
    const u64 *pa = digA + (size_t)slot * l;
    const u64 *pb = digB + (size_t)slot * l;
    constexpr u64 X80 = 0x8080808080808080ull;

    u64 amine[U], bmine[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {                      // blockDim * U == l: every thread owns U limbs
        const int m = u * c.nt + c.t;
        amine[u] = pa[m];
        bmine[u] = pb[m];
    }
    i64 d[1][2 * U];
    if (ta | tb) {
        // 2^N == -1: the product is -b, -a or 1 (MPIR's c flags, mul_fft.c:3250)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            if (ta && tb) {
                d[0][2 * u] = (m == 0) ? 1 : 0;
                d[0][2 * u + 1] = 0;
            } else {
                const u64 o = ta ? bmine[u] : amine[u];
                d[0][2 * u] = -(i64)(o & MPF_M32);
                d[0][2 * u + 1] = -(i64)(o >> 32);
            }
        }
    } else {
        // ---- stage the signed digits and the per-dword window sums --------------------
        for (int i = c.t; i < 8; i += c.nt) ((u32 *)SR)[i] = 0;
        for (int i = c.t; i < 16; i += c.nt) ((u32 *)(SR + 32 + L8))[i] = 0;
        for (int i = c.t; i < 256; i += c.nt) {
            ((u32 *)TB)[i] = 0;
            ((u32 *)(TB + 1024 + L8))[i] = 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            const u64 va = amine[u], vb = bmine[u];
            *(u64 *)(SR + 32 + L8 - 8 - 8 * m) = __builtin_bswap64(va ^ X80);
            *(u64 *)(TB + 1024 + 8 * m) = vb ^ X80;
            const int z0 = (int)__builtin_amdgcn_sad_u8((u32)va, 0, 0) + (int)__builtin_amdgcn_sad_u8((u32)vb, 0, 0);
            const int z1 = (int)__builtin_amdgcn_sad_u8((u32)(va >> 32), 0, 0) +
                           (int)__builtin_amdgcn_sad_u8((u32)(vb >> 32), 0, 0);
            PZ[2 * m] = z0 - 512;
            PZ[2 * m + 1] = z1 - 512;
        }
        __syncthreads();
        // exclusive prefix over the L32 dwords: thread t scans [2U t, 2U t + 2U)
        {
            int v[2 * U], run = 0;
#pragma unroll
            for (int k = 0; k < 2 * U; ++k) {
                v[k] = run;
                run += PZ[2 * U * c.t + k];
            }
            int x = run;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o);
                if (c.lane >= o) x += y;
            }
            if (c.lane == 63) wsum[c.wave] = x;
            __syncthreads();
            int base = x - run;
            for (int w = 0; w < c.wave; ++w) base += wsum[w];
#pragma unroll
            for (int k = 0; k < 2 * U; ++k) PZ[2 * U * c.t + k] = base + v[k];
            if (c.t == c.nt - 1) PZ[L32] = base + run;
        }
        __syncthreads();

        // ---- MFMA phase ------------------------------------------------------------------
        const int r = c.lane & 31, h = c.lane >> 5;
        const int oA = 32 + L8 - 1 - r + 16 * h;          // SR byte of A element j = 0 at d = 0
        const u32 sh = (u32)(oA & 3);
        const u32 *Ab = (const u32 *)(SR + (oA & ~3));     // - 8 dwords per d
        i64 F[FT][4];
        const i64 PZt = PZ[L32];
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
            const int p0 = 32 * (c.wave + ft * c.nw);
            const v4i_t *Blo = (const v4i_t *)(TB + 32 * (p0 + r + 32) + 16 * h);   // - 2 v4i per d
            const v4i_t *Bhi = Blo + 2 * NB;
            v16i_t lo = {}, hi = {};
            auto afrag = [&](int dd) {
                const u32 *ap = Ab - 8 * dd;
                const u32 w0 = ap[0], w1 = ap[1], w2 = ap[2], w3 = ap[3], w4 = ap[4];
                v4i_t a;
                a.x = (int)__builtin_amdgcn_alignbyte(w1, w0, sh);
                a.y = (int)__builtin_amdgcn_alignbyte(w2, w1, sh);
                a.z = (int)__builtin_amdgcn_alignbyte(w3, w2, sh);
                a.w = (int)__builtin_amdgcn_alignbyte(w4, w3, sh);
                return a;
            };
            for (int dd = 0; dd <= p0; ++dd)
                lo = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag(dd), Blo[-2 * dd], lo, 0, 0, 0);
            for (int dd = p0 + 1; dd <= p0 + 31; ++dd) {
                const v4i_t a = afrag(dd);
                lo = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, Blo[-2 * dd], lo, 0, 0, 0);
                hi = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, Bhi[-2 * dd], hi, 0, 0, 0);
            }
            for (int dd = p0 + 32; dd <= NB; ++dd)
                hi = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag(dd), Bhi[-2 * dd], hi, 0, 0, 0);
            // fold + window-sum correction: digit q = 8 p + 2 g + h of the residue
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q = 8 * (p0 + r) + 2 * g + h;
                const u32 u4 = __builtin_bswap32(*(const u32 *)(SR + 28 + L8 - 4 * q)) ^ 0x80808080u;
                const u32 v4 = *(const u32 *)(TB + 1024 + 4 * q) ^ 0x80808080u;
                i64 run = PZ[q], cz = 0, acc = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    run += (i64)((u4 >> (8 * e)) & 255) + (i64)((v4 >> (8 * e)) & 255) - 128;
                    cz += run << (8 * e);
                    acc += ((i64)lo[4 * g + e] - (i64)hi[4 * g + e]) << (8 * e);
                }
                F[ft][g] = acc + 128 * (2 * cz - PZt * (i64)0x01010101);
            }
        }
        __syncthreads();                                   // SR/TB dead: digits go to DG
        i64 *DG = (i64 *)smem;
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
            const int p0 = 32 * (c.wave + ft * c.nw);
#pragma unroll
            for (int g = 0; g < 4; ++g) DG[8 * (p0 + r) + 2 * g + h] = F[ft][g];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            d[0][2 * u] = DG[2 * m];
            d[0][2 * u + 1] = DG[2 * m + 1];
        }
    }
    long slots[1] = {slot};
    bool keep[1] = {true};
    normalize_store<U, 1>(c, d, slots, keep, false, st, l, sm);   // reduced: the inverse pass folds the carries
}


// --------------------------------------------------------------------------
// k_pwm2<U,T,D>: k_pwm with the MFMA operands register-blocked to cut LDS traffic.
// k_pwm reads one Toeplitz A fragment (5 dwords/lane) and one or two B fragments
// (16 B/lane) per MFMA, so it is bound by LDS bandwidth, not by the matrix cores.
// Here a wave owns T consecutive fold tiles p0_f = P0 + 32 f and walks the block
// distances dd in chains dd = k + 32 j (k < 32): for D consecutive j it loads the D
// A fragments A(k + 32 j) once and the B fragments by m = f - jj, since tile f at
// dd = k + 32 (j0 + jj) reads block P0 + r + 32 - k + 32 m (+ NB for hi) -- so T D
// lo MFMAs (and T D hi) need D A loads and T + D - 1 B loads each for lo and hi.
// Validity (which MFMAs k_pwm issues): lo iff dd <= p0_f + 31, hi iff p0_f + 1 <= dd
// <= NB; both depend on m only (plus dd <= NB on jj), and are wave-uniform.
// Same digit math, LDS layout and epilogue as k_pwm.  blockDim = 64 nw with
// nw T = NB / 32 fold tiles, U = l / blockDim.
// --------------------------------------------------------------------------
template <int U, int T, int D>
__global__ __launch_bounds__(D >= 4 ? 512 : 1024) void k_pwm2(u64 *digA, u64 *cbA, int *topA, const u64 *digB, const int *topB,
                                               int l, int ablate)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const int L8 = 8 * l, NB = l / 4, L32 = 2 * l;
    unsigned char *SR = smem;
    unsigned char *TB = SR + L8 + 96;
    int *PZ = (int *)(TB + L8 + 2048);
    int *wsum = PZ + ((L32 + 1) * 4 + 15) / 16 * 4;
    Lds sm;
    sm.stage = nullptr;
    sm.edge = wsum + 16;
    sm.scr = (u64 *)((unsigned char *)sm.edge + ((size_t)norm_edge_ints(1, U, c.nw) * sizeof(int) + 15) / 16 * 16);
    Coef st;
    st.dig = digA;
    st.cb = cbA;
    st.top = topA;
    const long slot = blockIdx.x;
    const int ta = topA[slot], tb = topB[slot];
    const u64 *pa = digA + (size_t)slot * l;
    const u64 *pb = digB + (size_t)slot * l;
    constexpr u64 X80 = 0x8080808080808080ull;

    u64 amine[U], bmine[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int m = u * c.nt + c.t;
        amine[u] = pa[m];
        bmine[u] = pb[m];
    }
    i64 d[1][2 * U];
    if (ta | tb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            if (ta && tb) {
                d[0][2 * u] = (m == 0) ? 1 : 0;
                d[0][2 * u + 1] = 0;
            } else {
                const u64 o = ta ? bmine[u] : amine[u];
                d[0][2 * u] = -(i64)(o & MPF_M32);
                d[0][2 * u + 1] = -(i64)(o >> 32);
            }
        }
    } else {
        for (int i = c.t; i < 8; i += c.nt) ((u32 *)SR)[i] = 0;
        for (int i = c.t; i < 16; i += c.nt) ((u32 *)(SR + 32 + L8))[i] = 0;
        for (int i = c.t; i < 256; i += c.nt) {
            ((u32 *)TB)[i] = 0;
            ((u32 *)(TB + 1024 + L8))[i] = 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            const u64 va = amine[u], vb = bmine[u];
            *(u64 *)(SR + 32 + L8 - 8 - 8 * m) = __builtin_bswap64(va ^ X80);
            *(u64 *)(TB + 1024 + 8 * m) = vb ^ X80;
            const int z0 = (int)__builtin_amdgcn_sad_u8((u32)va, 0, 0) + (int)__builtin_amdgcn_sad_u8((u32)vb, 0, 0);
            const int z1 = (int)__builtin_amdgcn_sad_u8((u32)(va >> 32), 0, 0) +
                           (int)__builtin_amdgcn_sad_u8((u32)(vb >> 32), 0, 0);
            PZ[2 * m] = z0 - 512;
            PZ[2 * m + 1] = z1 - 512;
        }
        __syncthreads();
        {
            int v[2 * U], run = 0;
#pragma unroll
            for (int k = 0; k < 2 * U; ++k) {
                v[k] = run;
                run += PZ[2 * U * c.t + k];
            }
            int x = run;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o);
                if (c.lane >= o) x += y;
            }
            if (c.lane == 63) wsum[c.wave] = x;
            __syncthreads();
            int base = x - run;
            for (int w = 0; w < c.wave; ++w) base += wsum[w];
#pragma unroll
            for (int k = 0; k < 2 * U; ++k) PZ[2 * U * c.t + k] = base + v[k];
            if (c.t == c.nt - 1) PZ[L32] = base + run;
        }
        __syncthreads();

        // ---- MFMA phase: T tiles x chains of D distances ---------------------------------
        const int r = c.lane & 31, h = c.lane >> 5;
        const int oA = 32 + L8 - 1 - r + 16 * h;
        const u32 sh = (u32)(oA & 3);
        const u32 *Ab = (const u32 *)(SR + (oA & ~3));
        const int P0 = 32 * T * c.wave;
        const v4i_t *Bb = (const v4i_t *)(TB + 32 * (P0 + r + 32) + 16 * h);   // block P0 + r (+32 pad)
        v16i_t lo[T], hi[T];
#pragma unroll
        for (int f = 0; f < T; ++f) {
            lo[f] = v16i_t{};
            hi[f] = v16i_t{};
        }
        auto afrag = [&](int dd) {
            const u32 *ap = Ab - 8 * dd;
            const u32 w0 = ap[0], w1 = ap[1], w2 = ap[2], w3 = ap[3], w4 = ap[4];
            v4i_t a;
            a.x = (int)__builtin_amdgcn_alignbyte(w1, w0, sh);
            a.y = (int)__builtin_amdgcn_alignbyte(w2, w1, sh);
            a.z = (int)__builtin_amdgcn_alignbyte(w3, w2, sh);
            a.w = (int)__builtin_amdgcn_alignbyte(w4, w3, sh);
            return a;
        };
        constexpr int NM = T + D - 1;   // m = f - jj in [-(D-1), T-1] -> index m + D - 1
        for (int k = 0; k < (ablate ? 0 : 32); ++k) {   // ablate: timing experiments only
            for (int j0 = 0; k + 32 * j0 <= NB; j0 += D) {
                v4i_t A[D];
#pragma unroll
                for (int jj = 0; jj < D; ++jj)
                    if (k + 32 * (j0 + jj) <= NB) A[jj] = afrag(k + 32 * (j0 + jj));
                v4i_t BL[NM], BH[NM];
#pragma unroll
                for (int mi = 0; mi < NM; ++mi) {
                    const int m = mi - (D - 1);
                    const int dm = k + 32 * (j0 - m);   // dd of the pair (f, jj) with f - jj = m
                    // some (f, jj) with f - jj = m, f < T, jj < D, dd <= NB
                    const int jlo = m < 0 ? -m : 0, jhi = (T - 1 - m) < (D - 1) ? (T - 1 - m) : (D - 1);
                    const bool any = jlo <= jhi && k + 32 * (j0 + jlo) <= NB;
                    const int boff = 32 * (m - j0) - k;   // in blocks, relative to Bb
                    if (any && dm <= P0 + 31) BL[mi] = Bb[2 * boff];
                    if (any && dm >= P0 + 1) BH[mi] = Bb[2 * boff + 2 * NB];
                }
#pragma unroll
                for (int f = 0; f < T; ++f)
#pragma unroll
                    for (int jj = 0; jj < D; ++jj) {
                        const int dd = k + 32 * (j0 + jj);
                        const int mi = f - jj + D - 1;
                        const int p0 = P0 + 32 * f;
                        if (dd <= NB) {
                            if (dd <= p0 + 31) lo[f] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[jj], BL[mi], lo[f], 0, 0, 0);
                            if (dd >= p0 + 1) hi[f] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[jj], BH[mi], hi[f], 0, 0, 0);
                        }
                    }
            }
        }
        i64 F[T][4];
        const i64 PZt = PZ[L32];
#pragma unroll
        for (int f = 0; f < T; ++f) {
            const int p0 = P0 + 32 * f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q = 8 * (p0 + r) + 2 * g + h;
                const u32 u4 = __builtin_bswap32(*(const u32 *)(SR + 28 + L8 - 4 * q)) ^ 0x80808080u;
                const u32 v4 = *(const u32 *)(TB + 1024 + 4 * q) ^ 0x80808080u;
                i64 run = PZ[q], cz = 0, acc = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    run += (i64)((u4 >> (8 * e)) & 255) + (i64)((v4 >> (8 * e)) & 255) - 128;
                    cz += run << (8 * e);
                    acc += ((i64)lo[f][4 * g + e] - (i64)hi[f][4 * g + e]) << (8 * e);
                }
                F[f][g] = acc + 128 * (2 * cz - PZt * (i64)0x01010101);
            }
        }
        __syncthreads();
        i64 *DG = (i64 *)smem;
#pragma unroll
        for (int f = 0; f < T; ++f) {
            const int p0 = P0 + 32 * f;
#pragma unroll
            for (int g = 0; g < 4; ++g) DG[8 * (p0 + r) + 2 * g + h] = F[f][g];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = u * c.nt + c.t;
            d[0][2 * u] = DG[2 * m];
            d[0][2 * u + 1] = DG[2 * m + 1];
        }
    }
    long slots[1] = {slot};
    bool keep[1] = {true};
    normalize_store<U, 1>(c, d, slots, keep, false, st, l, sm);
}
