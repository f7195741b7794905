// mpfft.hip -- host orchestration and C ABI of the MI355X-native new_mpn_mul.
//
// The drop-in boundary is new_mpn_mul(r1, i1, n1, i2, n2, depth, w)
// (the reference's mul_fft.c:3190-3191); see include/mpfft.h.  Everything below
// the boundary is a re-design for gfx950.  plan.hpp decides (Plan, the pointwise
// family, the chooser's cost model), exec.hpp launches (View, Exec); this file holds the stage
// profiling, the drivers, the per-device contexts and the C ABI.
//
//   1. forward column pass(es): split fused into the first pass; truncated DIF of
//      length NR on every column, both operands in one launch        (a2-a12)
//   2. forward row pass(es): MFA twiddle fused into the load, DIF of length NC
//      over the T/NC live rows, canonical store                       (a3, a7)
//   3. pointwise mulmod 2^N+1 over the T live slots                   (a20)
//   4. inverse row pass(es), MFA un-twiddle fused into the store      (a13, a15)
//   5. truncated inverse column transform (van der Hoeven), driven as a host
//      recursion of block IFFT passes and element-wise pair steps     (a13, a14)
//   6. scale by 2^-(depth+1) + canonicalise                           (a21)
//   7. combine: limb-parallel shifted sums + device-wide carry scan   (a22)
//
// Slot layout: operand X lives in slots 0..2n-1 (row-major, NC columns).  After
// stage 2, slot p*NC + q holds X_{revbin(p) + NR*revbin(q)} (the reference's
// slot map, mul_fft.c:2357, up to its two revbin permutations, which we never
// perform because the inverse undoes them).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "dot.hpp"
#include "combine.hpp"
#include "fold.hpp"
#include "sdot.hpp"
#include "nega.hpp"
#include "negaw.hpp"
#include "cyc.hpp"
#include "wdispatch.hpp"
#include "bdispatch.hpp"
#include "pdispatch.hpp"
#include "rdispatch.hpp"
#include "../../include/mpfft.h"
#include "plan.hpp"
#include "exec.hpp"

void mpfft_note_hip_error(hipError_t e) { last_hip_error = e; }   // multi.hip's failures

// multi.hip: the device list mpfft_set_devices / MPFFT_DEVICES picks for this product (0: none)
int mpfft_multi_policy(long n1, long n2, unsigned long depth, unsigned long w, std::vector<int> &devs);

// Stage profiling (mpfft_profile_begin/end): while active, each multiply claims a call slot
// and records a HIP event on its own stream at every stage boundary -- the timed calls are
// otherwise unchanged -- and profile_end sums the per-stage times of the calls that
// recorded every boundary.  A claimed slot keeps its own event pointer (taken under the
// lock), and profile_begin refuses to reallocate while claimed calls are still running.
struct StageProf {
    bool on = false;
    int cap = 0, used = 0, inflight = 0;
    hipEvent_t *ev = nullptr;   // cap * (MPFFT_NSTAGES + 1)
    int *marks = nullptr;       // per claimed call: boundaries recorded (MPFFT_NSTAGES + 1 = complete)
};
static std::mutex g_prof_mu;
static StageProf g_prof;

struct ProfCall {
    int call = -1;
    hipEvent_t *ev = nullptr;
    int marks = 0;
    ProfCall()
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (g_prof.on && g_prof.used < g_prof.cap) {
            call = g_prof.used++;
            ev = g_prof.ev + (size_t)call * (MPFFT_NSTAGES + 1);
            ++g_prof.inflight;
        }
    }
    void mark(int stage, hipStream_t s)
    {
        if (call < 0) return;
        if (hipEventRecord(ev[stage], s) == hipSuccess && stage == marks) ++marks;
    }
    ~ProfCall()
    {
        if (call < 0) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.marks[call] = marks;
        --g_prof.inflight;
    }
};

// the sqrt2 top level (kernels.hpp k_s2op): one workgroup per k in [k0, k0 + cnt)
static int s2_launch(const Plan &P, const Exec &X, int op, const u64 *srcA, const u64 *srcB, long k0, long cnt,
                     long tlo, int nops)
{
    if (cnt <= 0) return MPFFT_OK;
    S2Args a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < 2; ++k) {
        a.dig[k] = X.col.dig[k];
        a.cb[k] = X.col.cb[k];
        a.top[k] = X.col.top[k];
    }
    a.src[0] = srcA; a.nsrc[0] = P.n1;
    a.src[1] = srcB; a.nsrc[1] = P.n2;
    a.bits1 = P.bits1;
    a.N = P.N;
    a.w = (u64)P.w;
    a.l = (int)P.l;
    a.op = op;
    a.half = 2 * P.n;
    a.k0 = k0;
    a.tlo = tlo;
    void (*f)(S2Args) = nullptr;
    // l = 2048: four limbs per thread over 512 threads (k_s2op<2> at 1024 threads spilled 388 B)
    const int U = P.U == 2 && P.l == 2048 && !diag_env("MPFFT_S2_U2") ? 4 : P.U;
    const int tpb = (int)(P.l / U) < P.tpb ? (int)(P.l / U) : P.tpb;
    switch (U) {
    case 1: f = k_s2op<1>; break;
    case 2: f = k_s2op<2>; break;
    case 4: f = k_s2op<4>; break;
    }
    if (!f) return MPFFT_EUNSUPPORTED;
    const size_t lds = lds_bytes((int)P.l, s2_rb(U), 3, U, tpb / 64);
    allow_lds((const void *)f, lds);
    hipLaunchKernelGGL(f, dim3((unsigned)cnt, (unsigned)nops), dim3(tpb), lds, X.s, a);
    HIPCHK(hipGetLastError());
    return MPFFT_OK;
}

// new_mpn_mul6 (mul_fft.c:3573-3668) on the GPU: the sqrt2 top level (k_s2op) around two
// length-2n MFA multiplies that reuse every stage of run_all -- the first half full, the
// second truncated to trunc2 = Tr - NR rows (FFT/IFFT_radix2_mfa_truncate_sqrt2 :2212, :2593)
static int run_all6(const Plan &P, u64 *d_r, const u64 *d_i1, const u64 *d_i2, unsigned char *ws, hipStream_t s)
{
    Plan P1 = P, P2 = P, PS = P;
    P1.Tr = P.NR;
    P1.trunc = 2 * P.n;
    P2.Tr = P.Tr > P.NR ? P.Tr - P.NR : 0;
    P2.trunc = P2.Tr * P.NC;
    PS.depth = P.depth + 1;   // scale by 2^-(depth+2) (:3654-3658)
    Exec X1(P1, s), X2(P2, s), XS(PS, s), XC(P, s);
    X1.single(ws);
    X2.single(ws);
    X2.shift(2 * P.n);
    X2.in_rows = (int)P.NR;   // the second half's inputs are all live (FFT_radix2_truncate1_twiddle)
    X1.fuse_row_last = X2.fuse_row_last = true;   // each half's last row level inside its pointwise
    XS.single(ws);
    XC.single(ws);
    const bool two = P2.Tr > 0;
    const long tlo = P.trunc - 2 * P.n;   // pairs k < tlo carry both halves
    int rc;
    ProfCall pc;   // stage events as run_all's (the sqrt2 top level counts with the columns)
    pc.mark(0, s);
    if ((rc = s2_launch(P, X1, S2_FWD, d_i1, d_i2, 0, 2 * P.n, two ? 1 : 0, 2))) return rc;
    if ((rc = X1.fwd_columns(nullptr, 0, nullptr, 0, 2))) return rc;
    if (two && (rc = X2.fwd_columns(nullptr, 0, nullptr, 0, 2))) return rc;
    pc.mark(1, s);
    if ((rc = X1.fwd_rows(2))) return rc;
    if (two && (rc = X2.fwd_rows(2))) return rc;
    pc.mark(2, s);
    const bool fused = X1.row_fused() > 0;
    if ((rc = X1.pointwise())) return rc;
    if (two && (rc = X2.pointwise())) return rc;
    pc.mark(3, s);
    if (fused) {   // the products (and everything after) live in C: X1's views now start there
        XS.col = XS.row = X1.col;
        XC.col = XC.row = X1.col;
    }
    if ((rc = X1.inv_rows())) return rc;
    if (two && (rc = X2.inv_rows())) return rc;
    pc.mark(4, s);
    if ((rc = X1.itft(0, P.NR, P.NR))) return rc;
    if (two) {
        if ((rc = s2_launch(P, X1, S2_FILL, nullptr, nullptr, P2.Tr * P.NC, (P.NR - P2.Tr) * P.NC, 0, 1))) return rc;
        if ((rc = X2.itft1(0, P.NR, P2.Tr))) return rc;
    }
    if ((rc = s2_launch(P, X1, S2_IBFLY, nullptr, nullptr, 0, 2 * P.n, tlo > 0 ? tlo : 0, 1))) return rc;
    pc.mark(5, s);
    if ((rc = XS.scale())) return rc;
    pc.mark(6, s);
    rc = XC.combine_single(d_r, ws);
    pc.mark(7, s);
    return rc;
}

// Host operands (mul_host): operand 2's copy from the host runs on the context's copy stream
// while operand 1's forward columns and rows run on `s`; operand 2's passes wait for it.
struct HostB {
    const u64 *h;       // host limbs of operand 2 (null: d_i2 is already on the device)
    hipStream_t cs;     // copy stream
    hipEvent_t ready;   // recorded on cs after the copy
};

// operand 0 alone on a squaring plan and against a precomputed operand (one grid row), else both
// operands in one launch
static int fwd_nops(const Plan &P) { return P.sqr || P.pre ? 1 : 2; }
static int fwd_op(const Plan &P) { return P.sqr || P.pre ? 0 : -1; }

// The whole single-GPU product.  A squaring plan (make_plan_sqr) takes its operand as d_i1 and
// d_i2 alike: one split, one forward column and row transform (that pass still clears the
// combine flags), the pointwise in squaring mode (k_pwsq, or the other families with B = A),
// then the multiply's inverse, scaling and combine unchanged.
// A cyclic plan (make_plan_cyc, cyc.hpp: the product mod 2^B - 1, d_i1, d_i2 and d_r of L limbs) runs
// the same stages untruncated -- the split pass's zero bounds come out as "nothing pruned" -- and
// ends in the cyclic combine; its squares and cached operands work as the multiply's.
// d_pre: the cache of a precomputed operand B (plan_pre_bytes).  On a Plan::pre plan (make_plan_pre)
// the product is d_i1 times the cached operand: operand 0's forward stages, the pointwise against
// the cache, the rest unchanged.  pre_make (the multiply's own plan and workspace): operand B's
// forward columns and rows alone, then its row arrays into the cache (Exec::precomp_store) -- the
// stage marks after that one coincide.
static int run_all(const Plan &P, u64 *d_r, const u64 *d_i1, const u64 *d_i2, unsigned char *ws, hipStream_t s,
                   const HostB *hb = nullptr, unsigned char *d_pre = nullptr, bool pre_make = false)
{
    if (P.sqrt2) return run_all6(P, d_r, d_i1, d_i2, ws, s);
    Exec X(P, s);
    X.single(ws);
    X.use_pre(d_pre);
    X.pre_make = pre_make;
    X.zflags = X.comb_flags(ws);
    X.zflags_n = P.cyc ? Exec::cyc_flag_words(P) : X.comb_flag_words(P, P.total);   // cyclic: k_cwrap's behind them
    X.drive_single();
    X.fuse_row_last = true;  // last row level inside the pointwise (nested negacyclic sizes)
    ProfCall pc;
    int rc;
    pc.mark(0, s);
    if (pre_make) {
        // (operand B as both sources: its own zero bound prunes the split pass, operand 0 is not read)
        if ((rc = X.fwd_columns(d_i2, P.n2, d_i2, P.n2, 1, 1))) return rc;
        pc.mark(1, s);
        if ((rc = X.fwd_rows(1, 1))) return rc;
        pc.mark(2, s);
        rc = X.precomp_store();
        for (int k = 3; k <= MPFFT_NSTAGES; ++k) pc.mark(k, s);
        return rc;
    }
    if (hb && hb->h) {   // operand 1's forward transform overlaps operand 2's H2D copy
        // kernels first: a copy from pageable memory may hold the calling thread until it is done
        if ((rc = X.fwd_columns(d_i1, P.n1, d_i2, P.n2, 1, 0))) return rc;
        if ((rc = X.fwd_rows(1, 0))) return rc;
        HIPCHK(hipMemcpyAsync((void *)d_i2, hb->h, (size_t)P.n2 * 8, hipMemcpyHostToDevice, hb->cs));
        HIPCHK(hipEventRecord(hb->ready, hb->cs));
        HIPCHK(hipStreamWaitEvent(s, hb->ready, 0));
        if ((rc = X.fwd_columns(d_i1, P.n1, d_i2, P.n2, 1, 1))) return rc;
        if ((rc = X.fwd_rows(1, 1))) return rc;
        pc.mark(1, s);
    } else {
        if ((rc = X.fwd_columns(d_i1, P.n1, d_i2, P.n2, fwd_nops(P), fwd_op(P)))) return rc;
        pc.mark(1, s);
        if ((rc = X.fwd_rows(fwd_nops(P), fwd_op(P)))) return rc;
    }
    pc.mark(2, s);
    if ((rc = X.pointwise())) return rc;
    pc.mark(3, s);
    if ((rc = X.inv_rows())) return rc;
    pc.mark(4, s);
    if ((rc = X.itft(0, P.NR, P.Tr))) return rc;
    pc.mark(5, s);
    if ((rc = X.scale())) return rc;
    pc.mark(6, s);
    rc = P.cyc ? X.ccombine(d_r, ws) : X.fold ? X.combine_fold(d_r, ws, X.dbl_lo, X.dbl_hi) : X.combine_single(d_r, ws);
    pc.mark(7, s);
    return rc;
}

// The product mod 2^B + 1 on a make_plan_mod plan (nega.hpp): split + weight, the multiply's
// untruncated stages (the columns take slots, not operands), un-weight + scaling, negacyclic
// combine.  d_a, d_b: L + 1 limbs, fully reduced; d_r: L + 1 limbs.  Stage events as run_all's:
// the weight launch counts with the columns, the un-weight is the scaling stage.
static int run_all_mod(const Plan &P, u64 *d_r, const u64 *d_a, const u64 *d_b, unsigned char *ws, hipStream_t s)
{
    Exec X(P, s);
    X.single(ws);
    X.zflags = X.comb_flags(ws);   // cleared by the weight launch, with k_nwrap's behind them
    X.zflags_n = Exec::nega_flag_words(P);
    X.fuse_row_last = true;
    ProfCall pc;
    int rc;
    pc.mark(0, s);
    if ((rc = X.nweight(d_a, d_b, fwd_nops(P)))) return rc;
    if ((rc = X.fwd_columns(nullptr, 0, nullptr, 0, fwd_nops(P), fwd_op(P)))) return rc;
    pc.mark(1, s);
    if ((rc = X.fwd_rows(fwd_nops(P), fwd_op(P)))) return rc;
    pc.mark(2, s);
    if ((rc = X.pointwise())) return rc;   // a fused pointwise leaves X's views on C
    pc.mark(3, s);
    if ((rc = X.inv_rows())) return rc;
    pc.mark(4, s);
    if ((rc = X.itft(0, P.NR, P.NR))) return rc;
    pc.mark(5, s);
    if ((rc = X.unweight())) return rc;
    pc.mark(6, s);
    // the low-word CRT family (negaw.hpp): the low-word convolution counts with the combine stage
    if (P.lowcrt && (rc = X.nlowconv(d_a, d_b, ws))) return rc;
    rc = P.lowcrt ? X.ncombinew(d_r, ws) : X.ncombine(d_r, ws);
    pc.mark(7, s);
    return rc;
}

// The sum of K products on a make_plan_dot plan: per term the multiply's forward columns and rows of
// (a_i, b_i) and the pointwise into the C arrays -- the first term writes them, the later ones add
// to them (Exec::pointwise_dot) -- then the multiply's inverse rows, inverse columns, scaling and
// combine once, on C, for n1 + n2 + 1 limbs.  Where the pointwise works in place (every plan that
// fuses no row level), the first term's operand 0 is transformed in the C arrays themselves, so its
// product lands in C without a copy.  term(i, &a, &b): the device operands of term i (the host
// entries queue their copies there).
// Profiling: every term claims a call slot and marks its forward columns, rows and pointwise; the
// last term's slot carries the inverse side, the others mark those boundaries at once (empty
// stages) -- mpfft_profile_end's sums are the sum's stage times, its call count the terms.
// neg (mpfft_sdot_*, sdot.hpp): bit i set, term i is subtracted.  Its pre-pass (k_sdneg: ~a_i into the
// scratch behind the dot workspace, D <- D + b_i, the first one initialising D) is queued in front of
// its forward columns, which read the scratch in place of a_i, and counts with that stage; behind the
// combine, and counted with it, the correction d_r <- d_r + D - (D << 64 n1) (k_sdedge, k_sdfix).
// ws then has sd_layout's regions; neg == 0 launches neither and touches none of them.
template <typename Term>
static int run_dot(const Plan &P, long K, u64 *d_r, unsigned char *ws, hipStream_t s, Term term, u64 neg = 0)
{
    static_assert(SDFIX_CB == SD_FIX_BLOCK && SD_FIX_BLOCK == MPFFT_SDOT_FIX_BLOCK, "one chain block size");
    bool d_init = true;
    Exec X(P, s);
    X.single(ws);
    X.zflags = X.comb_flags(ws);
    X.zflags_n = X.comb_flag_words(P, P.total);
    X.drive_single();
    X.fuse_row_last = true;
    const View ab = X.col;
    const bool in_place = X.row_fused() == 0;
    int rc = MPFFT_OK;
    for (long i = 0; i < K; ++i) {
        const u64 *a = nullptr, *b = nullptr;
        ProfCall pc;
        pc.mark(0, s);
        if ((rc = term(i, &a, &b))) return rc;
        if ((neg >> i) & 1) {
            if ((rc = X.sd_neg(a, b, ws, d_init))) return rc;
            d_init = false;
            a = Exec::sd_scratch(P, ws);
        }
        X.col = X.row = ab;
        if (i == 0 && in_place) X.view_op0(X.cview);
        if ((rc = X.fwd_columns(a, P.n1, b, P.n2, 2))) return rc;
        pc.mark(1, s);
        if ((rc = X.fwd_rows(2))) return rc;
        pc.mark(2, s);
        if ((rc = X.pointwise_dot(i > 0))) return rc;
        pc.mark(3, s);
        if (i + 1 < K) {
            for (int k = 4; k <= MPFFT_NSTAGES; ++k) pc.mark(k, s);
            continue;
        }
        X.view_op0(X.cview);
        if ((rc = X.inv_rows())) return rc;
        pc.mark(4, s);
        if ((rc = X.itft(0, P.NR, P.Tr))) return rc;
        pc.mark(5, s);
        if ((rc = X.scale())) return rc;
        pc.mark(6, s);
        rc = X.fold ? X.combine_fold(d_r, ws, X.dbl_lo, X.dbl_hi) : X.combine_single(d_r, ws);
        if (!rc && neg) rc = X.sd_fix(d_r, ws);
        pc.mark(7, s);
    }
    return rc;
}

// The small matrix product R = X Y (mpfft_matmul_*; X m x k, Y k x p) on the dot plan at K = k and
// mm_layout's workspace.  Forward side, once per matrix entry: split, forward columns and forward rows
// of that operand alone -- X's entries as operand 0 in A's arrays, Y's as operand 1 in B's, each under
// its own zero-row bound -- then Exec::precomp_store into the entry's cache region (k_pwsx on nested
// plans, with the row levels the plan fuses).  Then per result entry: Exec::pointwise_mm writes C, and
// the multiply's inverse rows, truncated inverse columns, scaling and combine run on C into d_r[i p + j].
// What the inverse side of one entry assumes, and how each entry gets it:
//   * the combine's look-back flags and ticket counter are zero: no forward pass clears them here
//     (Exec::zflags stays null), so every combine clears its own in front of its launch;
//   * C's live slots hold this entry's pointwise sum: k_pwmm (or the first term's in-place product)
//     overwrites every live slot's limbs, carry masks and carry limb, nothing of the previous entry's
//     inverse is read;
//   * rows [Tr, NR) of C: the truncated inverse writes a row there (FILL) before it reads it;
//   * the deferred doubling's rows (dbl_lo, dbl_hi), the pending FILL and the chain are set by itft
//     itself on every call; the fold's meta words are written by k_cmeta in front of every combine;
//   * the row and column views point at C.
// opnd(e, &d): the device operand of matrix entry e (X's m k entries row-major, then Y's k p); the host
// entries queue its copy there.
// Profiling: every matrix entry claims a call slot and marks its forward columns and rows; its cache
// store counts as that slot's pointwise stage and the later boundaries are marked at once.  Every result
// entry claims a slot whose forward stages are empty and which carries the pointwise sum and the
// inverse side.  A product claims m k + k p + m p slots.
template <typename Opnd>
static int run_matmul(const Plan &P, int m, int k, int p, u64 *const *d_r, unsigned char *ws, hipStream_t s, Opnd opnd)
{
    static_assert(MM_MAX == MPFFT_MM_MAX, "one bound on the matrix dimensions");
    const MmLayout L = mm_layout(P, m, k, p);
    Exec X(P, s);
    X.single(ws);
    X.drive_single();
    X.fuse_row_last = true;
    X.pre_make = true;
    const View ab = X.col;
    int rc = MPFFT_OK;
    for (int e = 0; e < L.ncache; ++e) {
        const int op = e < m * k ? 0 : 1;
        const long n = op ? P.n2 : P.n1;
        const u64 *d = nullptr;
        ProfCall pc;
        pc.mark(0, s);
        if ((rc = opnd(e, &d))) return rc;
        X.pre = ws + L.off_cache + (size_t)e * L.stride;
        if ((rc = X.fwd_columns(d, n, d, n, 1, op))) return rc;
        pc.mark(1, s);
        if ((rc = X.fwd_rows(1, op))) return rc;
        pc.mark(2, s);
        if ((rc = X.precomp_store(op))) return rc;
        for (int st = 3; st <= MPFFT_NSTAGES; ++st) pc.mark(st, s);
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < p; ++j) {
            int ea[MM_MAX], eb[MM_MAX];
            for (int t = 0; t < k; ++t) {
                ea[t] = i * k + t;
                eb[t] = m * k + t * p + j;
            }
            ProfCall pc;
            for (int st = 0; st <= 2; ++st) pc.mark(st, s);
            X.col = X.row = ab;
            if ((rc = X.pointwise_mm(ws + L.off_cache, L.stride, k, ea, eb, false))) return rc;
            pc.mark(3, s);
            X.view_op0(X.cview);
            if ((rc = X.inv_rows())) return rc;
            pc.mark(4, s);
            if ((rc = X.itft(0, P.NR, P.Tr))) return rc;
            pc.mark(5, s);
            if ((rc = X.scale())) return rc;
            pc.mark(6, s);
            u64 *r = d_r[i * p + j];
            rc = X.fold ? X.combine_fold(r, ws, X.dbl_lo, X.dbl_hi) : X.combine_single(r, ws);
            pc.mark(7, s);
            if (rc) return rc;
        }
    return rc;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// The launches of the truncated inverse column transform as run_all drives it, one per line: a dry
// run of Exec::itft (Exec::rec), nothing touches the device.
static std::string inv_columns_launches(const Plan &P)
{
    std::string out;
    if (P.sqrt2) return out;
    Exec X(P, nullptr);
    X.single(nullptr);
    X.drive_single();
    X.rec = &out;
    if (X.itft(0, P.NR, P.Tr)) out.clear();
    return out;
}

// The launches of the forward column transform on whole operands, one per line (a dry run as above)
static std::string fwd_columns_launches(const Plan &P)
{
    std::string out;
    if (P.sqrt2) return out;
    static const u64 none = 0;   // a non-null operand pointer: the first pass splits (never read here)
    Exec X(P, nullptr);
    X.single(nullptr);
    X.drive_single();
    X.rec = &out;
    if (X.fwd_columns(&none, P.n1, &none, P.n2, 2)) out.clear();
    return out;
}

// Which kernel carries each stage of plan P (the same decisions Exec makes), seven fields joined
// by ';'.  On a squaring plan the pointwise is named k_pwsq<M>..., or "<kernel> (B = A)"; against
// a precomputed operand (Plan::pre) k_pwsp<M>..., or "<kernel> (B cached)".
static std::string stage_kernel_names(const Plan &P)
{
    const char *pass = P.big ? (P.rpass ? "k_rpass" : "k_bpass") : (P.wave && P.lds) ? "k_lpass" : P.wave ? "k_wpass" : "k_pass";
    const PwFamily fam = pw_family(P);
    const char *rows = P.big && P.rpass && fam != PWF_NESTED ? "k_rpass + k_bpass (canonical last pass)" : pass;
    char pw[112];
    if (fam == PWF_NESTED) {
        const int lk = pwss_lk_of(P.l);
        const char *fz = diag_env("MPFFT_FUSE_ROW");
        const bool fused = P.fuse_rows > 0 && !(fz && !strcmp(fz, "0"));   // as Exec::row_fused() in run_all
        snprintf(pw, sizeof pw, "%s<%d>%s (nested negacyclic, K=%d)", P.sqr ? "k_pwsq" : P.pre ? "k_pwsp" : "k_pwss", pw_inner_limbs(P.l, lk),
                 !fused ? "" : P.fuse_rows == 2 ? " quad + last two row levels" : " pair + last row level", 1 << lk);
    } else {
        snprintf(pw, sizeof pw, "%s%s", fam == PWF_PWM2 ? "k_pwm2 (int8 MFMA)" : fam == PWF_PWM ? "k_pwm (int8 MFMA)"
                                        : fam == PWF_PW ? "k_pw (VALU)" : "k_pointwise (VALU)", P.sqr ? " (B = A)" : P.pre ? " (B cached)" : "");
    }
    const char *pair = P.rpass ? "k_rpair" : P.wave ? "k_wpair" : "k_pairop";
    const char *scale = P.fuse_scale ? "(fused into the last inverse column pass)"
                        : P.fold ? "(folded: 2^-(depth+1) in the last inverse row pass)"
                        : P.rpass ? "k_rscale" : P.wave ? "k_wscale" : "k_scale";
    const char *comb = P.fold ? "k_cmeta + k_combine_red (reduced form)" : "k_combine1";
    // inverse columns: the FILL pass that also took the half-adds behind it is named with their distances
    char invc[96];
    int d1 = 0, d0 = 0;
    const std::string sched = inv_columns_launches(P);
    const size_t ha = sched.find(" halfadd ");
    if (ha != std::string::npos && sscanf(sched.c_str() + ha, " halfadd %d..%d", &d1, &d0) == 2)
        snprintf(invc, sizeof invc, "%s (FILL + half-add d=%d..%d) + %s", pass, d1, d0, pair);
    else
        snprintf(invc, sizeof invc, "%s + %s", pass, pair);
    // forward columns: where k_rpass also splits the operands, the first pass is named with its instance
    char fwdc[64];
    int fg = 0, fp = 0, fn = 0;
    if (sscanf(fwd_columns_launches(P).c_str(), "k_rpass<%d,%d,0,2>%n", &fg, &fp, &fn) == 2 && fn > 0)
        snprintf(fwdc, sizeof fwdc, "%s (split: k_rpass<%d,%d,0,2>)", pass, fg, fp);
    else
        snprintf(fwdc, sizeof fwdc, "%s", pass);
    if (P.cyc) {   // the cyclic top level (cyc.hpp): the first column pass splits, the fold is its own
        if (!(fn > 0)) snprintf(fwdc, sizeof fwdc, "%s (split)", pass);
        comb = "k_combine1 + k_cwrap + k_cfix (cyclic)";
    }
    if (P.nega) {   // the negacyclic top level's own launches (nega.hpp)
        Exec X(P, nullptr);
        char unw[64];
        snprintf(fwdc, sizeof fwdc, "k_nweight<%d> (split + weight) + %s", X.nega_u(), pass);
        if (X.unweight_rscale()) snprintf(unw, sizeof unw, "k_rscale (un-weight: exponent per slot)");
        else snprintf(unw, sizeof unw, "k_nunweight<%d>", X.nega_u());
        return std::string(fwdc) + ';' + rows + ';' + pw + ';' + pass + ';' + invc + ';' + unw + ';'
               + (P.lowcrt ? "k_nlowconv + k_combine1 + k_nwrapw + k_nfix (negacyclic, low-word CRT)"
                           : "k_combine1 + k_nwrap + k_nfix (negacyclic)");
    }
    return std::string(fwdc) + ';' + rows + ';' + pw + ';' + pass + ';' + invc + ';' + scale + ';' + comb;
}

// What writes the cache of a precomputed operand for the multiply's plan P: k_pwsx with the
// pointwise's pair / quad suffix, or a copy of B's row arrays
static std::string precomp_kernel_name(const Plan &P)
{
    if (pw_family(P) != PWF_NESTED) return "copy";
    const int lk = pwss_lk_of(P.l);
    const char *fz = diag_env("MPFFT_FUSE_ROW");
    const bool fused = P.has_c && !(fz && !strcmp(fz, "0"));   // as stage_kernel_names
    char pw[112];
    snprintf(pw, sizeof pw, "k_pwsx<%d>%s (nested negacyclic, K=%d)", pw_inner_limbs(P.l, lk),
             !fused ? "" : P.fuse_rows == 2 ? " quad + last two row levels" : " pair + last row level", 1 << lk);
    return pw;
}

// a whole string into the caller's buffer, or MPFFT_EINVAL
static int copy_out(const std::string &s, char *buf, size_t len)
{
    if (!buf || s.size() + 1 > len) return MPFFT_EINVAL;
    memcpy(buf, s.c_str(), s.size() + 1);
    return MPFFT_OK;
}

// what mpfft_plan_info and mpfft_workspace_layout report of a plan
static void plan_info_out(const Plan &P, long *out)
{
    out[0] = P.n; out[1] = P.l; out[2] = P.NC; out[3] = P.j1; out[4] = P.j2;
    out[5] = P.trunc; out[6] = (long)P.bits1; out[7] = P.NR; out[8] = P.tpb; out[9] = P.U;
}
static void layout_out(const Plan &P, size_t *out)
{
    out[0] = P.off_digA; out[1] = P.off_topA; out[2] = P.off_cbA;
    out[3] = P.off_digB; out[4] = P.off_topB; out[5] = P.off_cbB;   // 0 on a squaring plan: no B arrays
    out[6] = P.slots; out[7] = (size_t)cb_words((int)P.l);
}

// The plan queries of every entry family, behind its make_plan_*: rc is that call's status, P the plan it
// filled (read only where rc is 0).
static size_t bytes_or_0(int rc, const Plan &P) { return rc ? 0 : P.bytes; }
static int plan_info_out(int rc, const Plan &P, long *out)
{
    if (!rc) plan_info_out(P, out);
    return rc;
}
static int layout_out(int rc, const Plan &P, size_t *out)
{
    if (!rc) layout_out(P, out);
    return rc;
}
static int stage_names_out(int rc, const Plan &P, char *buf, size_t len)
{
    return rc ? rc : copy_out(stage_kernel_names(P), buf, len);
}

// The workspace precondition of a device or stage entry, checked behind the plan (else MPFFT_ENOMEM); the
// entry is about to launch
static bool ws_ok(const void *d_ws, size_t ws_bytes, size_t need)
{
    if (!d_ws || ws_bytes < need) return false;
    (void)hipGetLastError();  // clear a sticky error left by another library in this process
    return true;
}
// ... and that of a cache of operand 2: it holds the plan's forward transform (else MPFFT_ENOMEM)
static bool pre_ok(const void *d_pre, size_t pre_bytes, const Plan &P)
{
    return d_pre && pre_bytes >= plan_pre_bytes(P);
}

// The (depth, w) grid every chooser walks: depth 2 .. 24 and w = 1, 2, 4 .. 4096 with whole-limb coefficients
// of at most 4096 limbs.  make(&P, depth, w) builds a candidate's plan; *best is the valid one of least
// choose_cost, the first of equals.  False if no candidate is valid.
template <typename Make>
static bool search_grid(Plan *best, Make make)
{
    double cost = -1.0;
    for (unsigned long d = 2; d <= 24; ++d)
        for (unsigned long wv = 1; wv <= 4096; wv *= 2) {
            const unsigned long long N = (1ull << d) * wv;
            if (N % 64) continue;
            if (N / 64 > 4096) break;
            Plan P;
            if (make(&P, d, wv)) continue;
            const double c = choose_cost(P);
            if (cost < 0 || c < cost) {
                cost = c;
                *best = P;
            }
        }
    return cost >= 0;
}

// mpfft_choose's and mpfft_dot_choose's pick: that plan's (depth, w), or MPFFT_ETOOBIG
template <typename Make>
static int choose_on_grid(unsigned long *depth, unsigned long *w, Make make)
{
    Plan best;
    if (!search_grid(&best, make)) return MPFFT_ETOOBIG;
    *depth = (unsigned long)best.depth;
    *w = (unsigned long)best.w;
    return MPFFT_OK;
}

// One single-GPU stage (device pointers) on plan P; `ws` has P's workspace layout.  A squaring
// plan's forward stages run operand 0 alone.
static int single_stage(const Plan &P, int stage, const uint64_t *d_i1, const uint64_t *d_i2, uint64_t *d_r,
                        void *d_ws, size_t ws_bytes, void *stream, const void *d_pre = nullptr, bool from_c = false)
{
    const bool driven = (stage & MPFFT_STAGE_DRIVEN) != 0;   // (tests) the inverse stages as run_all drives them
    stage &= ~MPFFT_STAGE_DRIVEN;
    if (driven && stage != MPFFT_STAGE_INV_ROWS && stage != MPFFT_STAGE_INV_COLUMNS && stage != MPFFT_STAGE_SCALE)
        return MPFFT_EINVAL;
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    Exec X(P, (hipStream_t)stream);
    X.single((unsigned char *)d_ws);
    X.use_pre(d_pre);
    if (from_c) X.view_op0(X.cview);   // a dot plan's stages behind the pointwise: the accumulator
    if (driven) {
        X.drive_single();
        if (stage == MPFFT_STAGE_SCALE) plan_dbl(P, &X.dbl_lo, &X.dbl_hi);
    }
    switch (stage) {
    case MPFFT_STAGE_FWD_COLUMNS: return X.fwd_columns(d_i1, P.n1, d_i2, P.n2, fwd_nops(P), fwd_op(P));
    case MPFFT_STAGE_FWD_ROWS: return X.fwd_rows(fwd_nops(P), fwd_op(P));
    case MPFFT_STAGE_POINTWISE: return X.pointwise();
    case MPFFT_STAGE_INV_ROWS: return X.inv_rows();
    case MPFFT_STAGE_INV_COLUMNS: X.tail_fold = true; return X.itft(0, P.NR, P.Tr);
    case MPFFT_STAGE_SCALE: return X.scale();
    case MPFFT_STAGE_COMBINE: return X.combine_single(d_r, (unsigned char *)d_ws);
    case MPFFT_STAGE_FOLD_COMBINE: {
        if (!P.fold) return MPFFT_EUNSUPPORTED;
        long lo, hi;
        plan_dbl(P, &lo, &hi);
        return X.combine_fold(d_r, (unsigned char *)d_ws, lo, hi);
    }
    }
    return MPFFT_EINVAL;
}

// Fails loudly instead of segfaulting: the drop-in entries have no status to return
static void die_on(int rc, const char *fn, long n1, long n2, unsigned long depth, unsigned long w)
{
    if (!rc) return;
    fprintf(stderr, "%s(n1=%ld, n2=%ld, depth=%lu, w=%lu): %s\n", fn, n1, n2, depth, w, mpfft_strerror(rc));
    abort();
}

extern "C" {

int mpfft_inv_columns_schedule(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    return copy_out(inv_columns_launches(P), buf, len);
}

int mpfft_stage_kernels(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    snprintf(buf, len, "%s", stage_kernel_names(P).c_str());
    return MPFFT_OK;
}

int mpfft_profile_begin(int max_calls)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (max_calls < 1 || g_prof.inflight > 0) return MPFFT_EINVAL;
    const int per = MPFFT_NSTAGES + 1;
    if (g_prof.cap < max_calls) {
        for (int i = 0; i < g_prof.cap * per; ++i) (void)hipEventDestroy(g_prof.ev[i]);
        free(g_prof.ev);
        free(g_prof.marks);
        g_prof.cap = 0;
        g_prof.ev = (hipEvent_t *)calloc((size_t)max_calls * per, sizeof(hipEvent_t));
        g_prof.marks = (int *)calloc((size_t)max_calls, sizeof(int));
        if (!g_prof.ev || !g_prof.marks) return MPFFT_ENOMEM;
        for (int i = 0; i < max_calls * per; ++i)
            if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) {   // no leak: destroy what was made
                for (int j = 0; j < i; ++j) (void)hipEventDestroy(g_prof.ev[j]);
                return MPFFT_EHIP;
            }
        g_prof.cap = max_calls;
    }
    for (int c = 0; c < g_prof.cap; ++c) g_prof.marks[c] = 0;
    g_prof.used = 0;
    g_prof.on = true;
    return MPFFT_OK;
}

// sums the calls that recorded every stage boundary (a call that failed part-way is skipped)
int mpfft_profile_end(float *stage_ms, int *calls)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.on = false;
    for (int k = 0; k < MPFFT_NSTAGES; ++k) stage_ms[k] = 0.f;
    int done = 0;
    for (int c = 0; c < g_prof.used; ++c) {
        if (g_prof.marks[c] != MPFFT_NSTAGES + 1) continue;
        hipEvent_t *e = g_prof.ev + (size_t)c * (MPFFT_NSTAGES + 1);
        if (hipEventSynchronize(e[MPFFT_NSTAGES]) != hipSuccess) return MPFFT_EHIP;
        for (int k = 0; k < MPFFT_NSTAGES; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e[k], e[k + 1]) != hipSuccess) return MPFFT_EHIP;
            stage_ms[k] += ms;
        }
        ++done;
    }
    if (calls) *calls = done;
    return MPFFT_OK;
}

const char *mpfft_strerror(int code)
{
    switch (code) {
    case MPFFT_OK: return "ok";
    case MPFFT_EINVAL: return "invalid parameters (need n1,n2 >= 1, 2 <= depth <= 30, n*w % 64 == 0)"
                              "; mod 2^B+1: L >= 1, 2^(depth+1) | 64 L, operands fully reduced"
                              "; mod 2^B-1: L >= 1, 2^(depth+1) | 64 L, r overlapping no operand";
    case MPFFT_ETOOBIG: return "operands too large for the convolution: need j1 + j2 - 1 <= 2^(depth+1)"
                               "; mod 2^B+1: 2 bits1 + depth + 2 <= n*w, bits1 = 64 L / 2^(depth+1)"
                               "; mod 2^B-1: 2 bits1 + depth + 1 <= n*w";
    case MPFFT_EUNSUPPORTED: return "coefficient size n*w/64 > 4096 limbs is not supported";
    case MPFFT_ENOMEM: return "device allocation failed";
    case MPFFT_EHIP: return hipGetErrorString(last_hip_error);
    case MPFFT_ENODEV: return "no HIP device";
    }
    return "unknown error";
}

int mpfft_version(void) { return MPFFT_VERSION; }

int mpfft_check_params(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan(&P, n1, n2, depth, w);
}

size_t mpfft_workspace_bytes(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return bytes_or_0(make_plan(&P, n1, n2, depth, w), P);
}

int mpfft_workspace_layout(long n1, long n2, unsigned long depth, unsigned long w, size_t *out)
{
    Plan P;
    return layout_out(make_plan(&P, n1, n2, depth, w), P, out);
}

int mpfft_plan_info(long n1, long n2, unsigned long depth, unsigned long w, long *out)
{
    Plan P;
    return plan_info_out(make_plan(&P, n1, n2, depth, w), P, out);
}

// The multiply's driver on plan P (status rc) and the caller's workspace: the device entries of the plain,
// sqrt2, squaring, cached-operand and cyclic plans.  d_pre: the cache a Plan::pre plan reads, or with pre_make
// the one the multiply's plan writes.
static int device_run(int rc, const Plan &P, uint64_t *d_r, const uint64_t *d_i1, const uint64_t *d_i2, void *d_ws,
                      size_t ws_bytes, void *stream, const void *d_pre = nullptr, size_t pre_bytes = 0, bool pre_make = false)
{
    if (rc) return rc;
    if ((P.pre || pre_make) && !pre_ok(d_pre, pre_bytes, P)) return MPFFT_ENOMEM;
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    return run_all(P, d_r, d_i1, d_i2, (unsigned char *)d_ws, (hipStream_t)stream, nullptr, (unsigned char *)d_pre, pre_make);
}

int mpfft_mul_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const uint64_t *d_i2, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan(&P, n1, n2, depth, w), P, d_r, d_i1, d_i2, d_ws, ws_bytes, stream);
}

// stage entry points (device pointers), used by the stage-parity tests and the
// multi-GPU driver.  `ws` has the single-GPU workspace layout for (n1, n2, depth, w).
int mpfft_stage(int stage, const uint64_t *d_i1, const uint64_t *d_i2, uint64_t *d_r, long n1, long n2,
                unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    return single_stage(P, stage, d_i1, d_i2, d_r, d_ws, ws_bytes, stream);
}

// ---- sharded multi-GPU stages ------------------------------------------------
static int shard_exec(Exec &X, const mpfft_shard *sh)
{
    const Plan &P = X.P;
    if (sh->ccount < 1 || sh->c0 < 0 || sh->c0 + sh->ccount > P.NC) return MPFFT_EINVAL;
    if (sh->rcount < 0 || sh->r0 < 0 || sh->r0 + sh->rcount > P.Tr) return MPFFT_EINVAL;
    if (sh->ccb < 1 || P.NC % sh->ccb || (sh->ccb & (sh->ccb - 1))) return MPFFT_EINVAL;
    for (int k = 0; k < 2; ++k) {
        X.col.dig[k] = sh->col_dig[k];
        X.col.cb[k] = sh->col_cb[k];
        X.col.top[k] = sh->col_top[k];
        X.row.dig[k] = sh->row_dig[k];
        X.row.cb[k] = sh->row_cb[k];
        X.row.top[k] = sh->row_top[k];
    }
    X.c0 = sh->c0;
    X.ccount = sh->ccount;
    X.r0 = sh->r0;
    X.rcount = sh->rcount;
    X.ccb = sh->ccb;
    X.cbb = ilog2(sh->ccb);
    X.cbs = (long)sh->rcount * sh->ccb;
    X.src_chunk = sh->src_chunk;
    if (sh->rowc_dig && sh->rowc_cb && sh->rowc_top) {   // fused last row level (mpfft_shard_row_fused)
        X.cview.dig[0] = sh->rowc_dig;
        X.cview.cb[0] = sh->rowc_cb;
        X.cview.top[0] = sh->rowc_top;
        X.fuse_row_last = true;
    }
    return MPFFT_OK;
}

// The row stages on local rows [lo, hi) only (a row chunk: its exchange #2 can start while the
// next chunk computes).  The row layout keeps its block stride (rcount ccb slots per column
// block); the row passes take the chunk through their row offset and count, the pointwise is
// launched once per column block on the chunk's contiguous slots.
int mpfft_shard_stage_rows(int stage, const mpfft_shard *sh, int lo, int hi, void *stream)
{
    Plan P;
    int rc = make_plan(&P, sh->n1, sh->n2, sh->depth, sh->w);
    if (rc) return rc;
    if (lo < 0 || hi > sh->rcount || lo > hi) return MPFFT_EINVAL;
    if (stage != MPFFT_SHARD_FWD_ROWS && stage != MPFFT_SHARD_POINTWISE && stage != MPFFT_SHARD_INV_ROWS)
        return MPFFT_EINVAL;
    if (lo == hi) return MPFFT_OK;
    (void)hipGetLastError();
    Exec X(P, (hipStream_t)stream);
    if ((rc = shard_exec(X, sh))) return rc;
    // X.cbs (the block stride) stays the full rcount ccb
    X.row.advance((long)lo * X.ccb, P.l);
    X.cview.advance((long)lo * X.ccb, P.l);
    X.r0 += lo;
    X.rcount = hi - lo;
    if (stage == MPFFT_SHARD_FWD_ROWS) return X.fwd_rows(2);
    if (stage == MPFFT_SHARD_INV_ROWS) return X.inv_rows();
    for (long b = 0; b < P.NC / X.ccb; ++b) {   // the pointwise: one launch per column block
        Exec Y = X;
        Y.row.advance(b * X.cbs, P.l);
        Y.cview.advance(b * X.cbs, P.l);
        Y.pw_count = (long)(hi - lo) * X.ccb;
        if ((rc = Y.pointwise())) return rc;
    }
    return MPFFT_OK;
}

int mpfft_shard_row_fused(long n1, long n2, unsigned long depth, unsigned long w, int ccb)
{
    Plan P;
    if (make_plan(&P, n1, n2, depth, w)) return 0;
    return P.has_c && pw_pair_kernel(P.l, P.fuse_rows) && ccb >= (1 << P.fuse_rows) && !(P.NC % ccb);
}

int mpfft_shard_stage(int stage, const mpfft_shard *sh, const uint64_t *d_i1, const uint64_t *d_i2, void *stream)
{
    Plan P;
    int rc = make_plan(&P, sh->n1, sh->n2, sh->depth, sh->w);
    if (rc) return rc;
    (void)hipGetLastError();
    Exec X(P, (hipStream_t)stream);
    if ((rc = shard_exec(X, sh))) return rc;
    switch (stage) {
    case MPFFT_SHARD_FWD_COLUMNS: return X.fwd_columns(d_i1, sh->n1, d_i2, sh->n2, 2);
    case MPFFT_SHARD_FWD_COLUMNS_A: return X.fwd_columns(d_i1, sh->n1, d_i2, sh->n2, 2, 0);
    case MPFFT_SHARD_FWD_COLUMNS_B: return X.fwd_columns(d_i1, sh->n1, d_i2, sh->n2, 2, 1);
    case MPFFT_SHARD_FWD_COLUMNS_OWN:
        X.own_lo = sh->r0;
        X.own_hi = sh->r0 + sh->rcount;
        return X.fwd_columns(d_i1, sh->n1, d_i2, sh->n2, 2);
    case MPFFT_SHARD_FWD_ROWS: return X.rcount ? X.fwd_rows(2) : MPFFT_OK;
    case MPFFT_SHARD_POINTWISE: return X.pointwise();
    case MPFFT_SHARD_INV_ROWS: return X.rcount ? X.inv_rows() : MPFFT_OK;
    case MPFFT_SHARD_INV_COLUMNS:
        X.defer_double = true;
        if ((rc = X.itft(0, P.NR, P.Tr))) return rc;
        return X.scale();
    }
    return MPFFT_EINVAL;
}

// the stripes of one rank of the column-sharded multiply (multi.hip mpfft_shard_partition):
// stripe j of rank g (g = c0 / ccount of G = NC / ccount ranks) is product stripe j G + g,
// coefficients [(j G + g) C, + C) = column-layout row j of the rank
static void shard_comb_args(const Plan &P, const mpfft_shard *sh, CombArgs *a, long *nst, long *stripe_limbs)
{
    memset(a, 0, sizeof(*a));
    a->C = sh->ccount;
    a->G = (int)(P.NC / sh->ccount);
    a->g = sh->c0 / sh->ccount;
    a->S = (long)a->G * P.Tr;
    *nst = P.Tr;
    // limbs of a stripe at most: ms(s+1) - ms(s) <= ceil(C bits1 / 64); the last stripe runs to
    // the product's end, 64 total <= (len + 1) bits1 <= (T + 1) bits1: at most (C + 1) bits1 / 64 + 2
    *stripe_limbs = (long)((((u64)sh->ccount + 1) * P.bits1) / 64) + 2;
}

size_t mpfft_shard_combine_tmp_bytes(long n1, long n2, unsigned long depth, unsigned long w, int world)
{
    Plan P;
    if (make_plan(&P, n1, n2, depth, w) || world < 1 || P.NC % world) return 0;
    const long sl = (long)((((u64)(P.NC / world) + 1) * P.bits1) / 64) + 2;
    const long nb = P.Tr * Exec::comb_blocks(P, sl);
    return align_up((size_t)(nb + 1) * 4, 256) + align_up((size_t)nb * 4, 256);
}

int mpfft_shard_combine(const mpfft_shard *sh, int phase, uint64_t *d_r, const uint64_t *d_halo, int *d_sums,
                        const int *d_sums_all, void *d_tmp, size_t tmp_bytes, void *stream)
{
    Plan P;
    int rc = make_plan(&P, sh->n1, sh->n2, sh->depth, sh->w);
    if (rc) return rc;
    if (sh->ccount < 1 || P.NC % sh->ccount || sh->c0 % sh->ccount) return MPFFT_EINVAL;
    const int world = (int)(P.NC / sh->ccount);
    if (tmp_bytes < mpfft_shard_combine_tmp_bytes(sh->n1, sh->n2, sh->depth, sh->w, world)) return MPFFT_ENOMEM;
    const long H = (long)((P.N + 128 + P.bits1 - 1) / P.bits1) + 1;
    if (phase == 0 && (!d_sums || (!d_halo && (long)world * P.Tr > 1))) return MPFFT_EINVAL;
    if (phase == 1 && !d_sums_all) return MPFFT_EINVAL;
    (void)hipGetLastError();
    Exec X(P, (hipStream_t)stream);
    if ((rc = shard_exec(X, sh))) return rc;
    CombArgs a;
    long nst, sl;
    shard_comb_args(P, sh, &a, &nst, &sl);
    a.dig = X.col.dig[0];
    a.halo = d_halo;
    a.H = (int)H;
    a.SL = sl;
    const long nb = nst * Exec::comb_blocks(P, sl);
    u32 *st = (u32 *)d_tmp;
    u32 *allp = (u32 *)((unsigned char *)d_tmp + align_up((size_t)(nb + 1) * 4, 256));
    hipStream_t s = (hipStream_t)stream;
    if (phase == 0) {   // every stripe with carry-in 0, and its (generate, propagate) summary
        if ((rc = X.combine1(a, nst, sl, d_r, st, false, allp))) return rc;
        hipLaunchKernelGGL(k_comb_summary, dim3((unsigned)nst), dim3(256), 0, s, (const u32 *)st, (const u32 *)allp,
                           Exec::comb_blocks(P, sl), d_sums);
        HIPCHK(hipGetLastError());
        return MPFFT_OK;
    }
    // the carries between stripes, from every rank's summaries
    a.l = (int)P.l;
    a.N = P.N;
    a.bits1 = P.bits1;
    a.len = P.len;
    a.total = P.total;
    hipLaunchKernelGGL(k_stripe_carry, dim3((unsigned)nst), dim3(256), 0, s, a, nst, d_sums_all, d_r);
    HIPCHK(hipGetLastError());
    return MPFFT_OK;
}

// host-pointer entry with status.  One context per device (SURVEY 8b "Threading"):
// the calling thread's current HIP device selects it, so threads driving different
// GPUs never share memory or streams; threads on the same device serialise on its lock.
struct DevCtx {
    std::mutex mu;
    unsigned char *ws = nullptr;
    size_t ws_bytes = 0;
    u64 *io = nullptr;
    size_t io_bytes = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy = nullptr;   // operand 2's H2D beside operand 1's forward transform
    hipEvent_t ready = nullptr;
};
static const int MPFFT_MAX_DEV = 64;
static DevCtx g_dev[MPFFT_MAX_DEV];

// grow-only device buffer owned by a DevCtx
static int ensure_buf(void **p, size_t *have, size_t need)
{
    if (*have >= need) return MPFFT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipMalloc(p, need) != hipSuccess) return MPFFT_ENOMEM;
    *have = need;
    return MPFFT_OK;
}

// One host-pointer call on the calling thread's device: open() finds the device's context, holds its lock
// until the call returns, makes the context's stream on first use and grows its ws and io buffers to the
// sizes stated.  copy: the copy stream and its event too.  on_dev >= 0: MPFFT_EINVAL on any other device.
namespace {
struct HostCall {
    DevCtx *C = nullptr;
    int dev = 0;
    std::unique_lock<std::mutex> lk;
    int open(size_t ws_bytes, size_t io_bytes, bool copy = false, int on_dev = -1)
    {
        int ndev = 0, rc;
        (void)hipGetLastError();
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MPFFT_ENODEV;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MPFFT_MAX_DEV) return MPFFT_ENODEV;
        if (on_dev >= 0 && dev != on_dev) return MPFFT_EINVAL;
        C = &g_dev[dev];
        lk = std::unique_lock<std::mutex>(C->mu);
        if (!C->stream) HIPCHK(hipStreamCreateWithFlags(&C->stream, hipStreamNonBlocking));
        if (copy) {
            if (!C->copy) HIPCHK(hipStreamCreateWithFlags(&C->copy, hipStreamNonBlocking));
            if (!C->ready) HIPCHK(hipEventCreateWithFlags(&C->ready, hipEventDisableTiming));
        }
        if ((rc = ensure_buf((void **)&C->ws, &C->ws_bytes, ws_bytes))) return rc;
        return ensure_buf((void **)&C->io, &C->io_bytes, io_bytes);
    }
};
}  // namespace

// Host operands on the calling thread's device: io holds the operands and, behind them, the
// n1 + n2 result limbs.  A squaring plan (i2 == i1, n2 == n1) copies its one operand on the
// context's stream and needs no copy stream and no event.
static int mul_host(const Plan &P, uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2)
{
    int rc;
    HostCall H;
    const long nin = P.sqr ? n1 : n1 + n2;
    if ((rc = H.open(P.bytes, (size_t)(nin + n1 + n2) * 8, !P.sqr))) return rc;
    DevCtx &C = *H.C;
    u64 *d_i1 = C.io, *d_i2 = P.sqr ? d_i1 : d_i1 + n1, *d_r = C.io + nin;
    HIPCHK(hipMemcpyAsync(d_i1, i1, (size_t)n1 * 8, hipMemcpyHostToDevice, C.stream));
    HostB hb{P.sqrt2 || P.sqr ? nullptr : i2, C.copy, C.ready};
    if (P.sqrt2) HIPCHK(hipMemcpyAsync(d_i2, i2, (size_t)n2 * 8, hipMemcpyHostToDevice, C.stream));
    rc = run_all(P, d_r, d_i1, d_i2, C.ws, C.stream, &hb);
    if (rc) {
        if (!P.sqr) (void)hipStreamSynchronize(C.copy);   // the copy stream never outlives the call
        return rc;
    }
    HIPCHK(hipMemcpyAsync(r1, d_r, (size_t)(n1 + n2) * 8, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipStreamSynchronize(C.stream));
    return MPFFT_OK;
}

static thread_local int g_last_ngpus = 0;
int mpfft_last_ngpus(void) { return g_last_ngpus; }

int mpfft_mul_ex(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2, unsigned long depth,
                 unsigned long w)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    std::vector<int> devs;
    if (mpfft_multi_policy(n1, n2, depth, w, devs) > 1) {   // column-sharded over the policy's devices
        g_last_ngpus = (int)devs.size();
        rc = mpfft_mul_multi(r1, i1, n1, i2, n2, depth, w, (int)devs.size(), devs.data());
        // the policy's devices missing or full: the product still fits one device
        if (rc != MPFFT_ENODEV && rc != MPFFT_ENOMEM) return rc;
    }
    g_last_ngpus = 1;
    return mul_host(P, r1, i1, n1, i2, n2);
}

// ---- the sqrt2 front end new_mpn_mul6 (mul_fft.c:3573-3668) ---------
int mpfft_check_params6(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan(&P, n1, n2, depth, w, true);
}

size_t mpfft_workspace_bytes6(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return bytes_or_0(make_plan(&P, n1, n2, depth, w, true), P);
}

int mpfft_plan_info6(long n1, long n2, unsigned long depth, unsigned long w, long *out)
{
    Plan P;
    return plan_info_out(make_plan(&P, n1, n2, depth, w, true), P, out);
}

int mpfft_mul6_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const uint64_t *d_i2, long n2,
                      unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan(&P, n1, n2, depth, w, true), P, d_r, d_i1, d_i2, d_ws, ws_bytes, stream);
}

int mpfft_mul6_ex(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2, unsigned long depth,
                  unsigned long w)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w, true);
    if (rc) return rc;
    return mul_host(P, r1, i1, n1, i2, n2);
}

// mul_fft.c:3573 -- same signature and meaning; fails loudly instead of segfaulting
void new_mpn_mul6(mp_limb_t *r1, mp_limb_t *i1, mp_size_t n1, mp_limb_t *i2, mp_size_t n2, mp_bitcnt_t depth,
                  mp_bitcnt_t w)
{
    die_on(mpfft_mul6_ex(r1, i1, n1, i2, n2, depth, w), "new_mpn_mul6", (long)n1, (long)n2, depth, w);
}

// ---- squaring entries: the multiply's drivers on a squaring plan (make_plan_sqr), the one
// operand passed as both.  Out of scope: the sqrt2 front end (new_mpn_mul6), the sharded and
// multi-GPU entries and mpfft_set_devices routing -- a square always runs on the calling
// thread's device. -----------------------------------------------------------------------
size_t mpfft_sqr_workspace_bytes(long n, unsigned long depth, unsigned long w)
{
    Plan P;
    return bytes_or_0(make_plan_sqr(&P, n, depth, w), P);
}

int mpfft_sqr_workspace_layout(long n, unsigned long depth, unsigned long w, size_t *out)
{
    Plan P;
    return layout_out(make_plan_sqr(&P, n, depth, w), P, out);
}

int mpfft_sqr_device(uint64_t *d_r, const uint64_t *d_a, long n, unsigned long depth, unsigned long w,
                     void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan_sqr(&P, n, depth, w), P, d_r, d_a, d_a, d_ws, ws_bytes, stream);
}

int mpfft_sqr_stage(int stage, const uint64_t *d_a, uint64_t *d_r, long n, unsigned long depth,
                    unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan_sqr(&P, n, depth, w);
    if (rc) return rc;
    return single_stage(P, stage, d_a, d_a, d_r, d_ws, ws_bytes, stream);
}

int mpfft_sqr_stage_kernels(long n, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P;
    return stage_names_out(make_plan_sqr(&P, n, depth, w), P, buf, len);
}

// host-pointer square: never routed by mpfft_set_devices
int mpfft_sqr_ex(uint64_t *r, const uint64_t *a, long n, unsigned long depth, unsigned long w)
{
    Plan P;
    int rc = make_plan_sqr(&P, n, depth, w);
    if (rc) return rc;
    if ((rc = mul_host(P, r, a, n, a, n))) return rc;
    g_last_ngpus = 1;
    return MPFFT_OK;
}

// ---- multiplication by a precomputed operand: operand 2's forward transform is computed once
// into a cache (run_all's pre_make mode on the multiply's plan), and each product against it runs
// the multiply's driver on the plan without B's arrays (make_plan_pre), the pointwise reading the
// cache.  Out of scope as for the squares: the sqrt2 front end, the mod 2^B + 1 entries, the
// sharded and multi-GPU entries, mpfft_set_devices routing. -----------------------------------
size_t mpfft_precomp_bytes(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    if (make_plan(&P, n1, n2, depth, w)) return 0;
    return plan_pre_bytes(P);
}

int mpfft_precomp_device(void *d_pre, size_t pre_bytes, const uint64_t *d_i2, long n1, long n2, unsigned long depth,
                         unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan(&P, n1, n2, depth, w), P, nullptr, nullptr, d_i2, d_ws, ws_bytes, stream, d_pre, pre_bytes, true);
}

size_t mpfft_mul_precomp_workspace_bytes(long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return bytes_or_0(make_plan_pre(&P, n1, n2, depth, w), P);
}

int mpfft_mul_precomp_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const void *d_pre, size_t pre_bytes, long n2,
                             unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan_pre(&P, n1, n2, depth, w), P, d_r, d_i1, d_i1, d_ws, ws_bytes, stream, d_pre, pre_bytes);
}

int mpfft_precomp_stage_kernels(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P, Q;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc || (rc = make_plan_pre(&Q, n1, n2, depth, w))) return rc;
    return copy_out(precomp_kernel_name(P) + ';' + stage_kernel_names(Q), buf, len);
}

int mpfft_precomp_stage(int stage, void *d_pre, size_t pre_bytes, const uint64_t *d_i2, long n1, long n2,
                        unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    if (stage != MPFFT_STAGE_FWD_COLUMNS && stage != MPFFT_STAGE_FWD_ROWS && stage != MPFFT_STAGE_PRE_STORE)
        return MPFFT_EINVAL;
    if (stage == MPFFT_STAGE_PRE_STORE && !pre_ok(d_pre, pre_bytes, P)) return MPFFT_ENOMEM;
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    Exec X(P, (hipStream_t)stream);
    X.single((unsigned char *)d_ws);
    X.use_pre(d_pre);
    X.pre_make = true;
    if (stage == MPFFT_STAGE_FWD_COLUMNS) return X.fwd_columns(d_i2, P.n2, d_i2, P.n2, 1, 1);
    if (stage == MPFFT_STAGE_FWD_ROWS) return X.fwd_rows(1, 1);
    return X.precomp_store();
}

int mpfft_mul_precomp_stage(int stage, const uint64_t *d_i1, const void *d_pre, size_t pre_bytes, uint64_t *d_r, long n1,
                            long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan_pre(&P, n1, n2, depth, w);
    if (rc) return rc;
    if ((stage & ~MPFFT_STAGE_DRIVEN) == MPFFT_STAGE_POINTWISE && !pre_ok(d_pre, pre_bytes, P)) return MPFFT_ENOMEM;
    return single_stage(P, stage, d_i1, d_i1, d_r, d_ws, ws_bytes, stream, d_pre);
}

// host pointers: the handle owns the device cache, made on the calling thread's device
struct mpfft_pre {
    int dev;
    long n1, n2;
    unsigned long depth, w;
    int family;     // the pointwise family (MPFFT_POINTWISE) the cache was made for
    void *d_pre;
    size_t bytes;
};

int mpfft_precomp_create(mpfft_pre **out, const uint64_t *i2, long n2, long n1, unsigned long depth, unsigned long w)
{
    if (!out) return MPFFT_EINVAL;
    *out = nullptr;
    Plan P;
    int rc = make_plan(&P, n1, n2, depth, w);
    if (rc) return rc;
    HostCall H;
    if ((rc = H.open(P.bytes, (size_t)n2 * 8))) return rc;
    DevCtx &C = *H.C;
    mpfft_pre *h = new mpfft_pre{H.dev, n1, n2, depth, w, (int)pw_family(P), nullptr, plan_pre_bytes(P)};
    if (hipMalloc(&h->d_pre, h->bytes) != hipSuccess) {
        delete h;
        return MPFFT_ENOMEM;
    }
    rc = hipMemcpyAsync(C.io, i2, (size_t)n2 * 8, hipMemcpyHostToDevice, C.stream) == hipSuccess ? MPFFT_OK : MPFFT_EHIP;
    if (!rc) rc = run_all(P, nullptr, nullptr, C.io, C.ws, C.stream, nullptr, (unsigned char *)h->d_pre, true);
    if (!rc && hipStreamSynchronize(C.stream) != hipSuccess) rc = MPFFT_EHIP;
    if (rc) {
        if (rc == MPFFT_EHIP) last_hip_error = hipGetLastError();
        (void)hipFree(h->d_pre);
        delete h;
        return rc;
    }
    *out = h;
    return MPFFT_OK;
}

int mpfft_mul_precomp_ex(uint64_t *r, const uint64_t *i1, long n1, const mpfft_pre *pre)
{
    if (!pre || n1 != pre->n1) return MPFFT_EINVAL;
    Plan P;
    int rc = make_plan_pre(&P, n1, pre->n2, pre->depth, pre->w);
    if (rc) return rc;
    if ((int)pw_family(P) != pre->family) return MPFFT_EINVAL;   // MPFFT_POINTWISE changed since the cache was made
    const long n2 = pre->n2;
    HostCall H;
    if ((rc = H.open(P.bytes, (size_t)(2 * n1 + n2) * 8, false, pre->dev))) return rc;   // the cache's device only
    DevCtx &C = *H.C;
    u64 *d_i1 = C.io, *d_r = C.io + n1;
    HIPCHK(hipMemcpyAsync(d_i1, i1, (size_t)n1 * 8, hipMemcpyHostToDevice, C.stream));
    if ((rc = run_all(P, d_r, d_i1, d_i1, C.ws, C.stream, nullptr, (unsigned char *)pre->d_pre))) return rc;
    HIPCHK(hipMemcpyAsync(r, d_r, (size_t)(n1 + n2) * 8, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipStreamSynchronize(C.stream));
    g_last_ngpus = 1;
    return MPFFT_OK;
}

void mpfft_precomp_destroy(mpfft_pre *pre)
{
    if (!pre) return;
    if (pre->d_pre) (void)hipFree(pre->d_pre);
    delete pre;
}

// ---- products mod 2^B + 1 (nega.hpp, make_plan_mod, run_all_mod).  Out of scope as for the
// squares: the sqrt2 front end, the sharded and multi-GPU entries, mpfft_set_devices routing.
// Two entry families over the same code, told apart by make_plan_mod's crt: mpfft_mulmod_* (the
// signs read back from the residues) and mpfft_mulmodw_* (the low-word CRT, negaw.hpp; the cached
// operand is out of scope there too). -------------------------------------------------------------
} // extern "C"

static size_t mod_workspace_bytes(long L, unsigned long depth, unsigned long w, int sqr, bool crt)
{
    Plan P;
    return bytes_or_0(make_plan_mod(&P, L, depth, w, sqr != 0, crt), P);
}

static int mod_plan_info(long L, unsigned long depth, unsigned long w, long *out, bool crt)
{
    Plan P;
    return plan_info_out(make_plan_mod(&P, L, depth, w, false, crt), P, out);
}

// out[8], and on the low-word CRT family out[8]: the byte offset of d
static int mod_workspace_layout(long L, unsigned long depth, unsigned long w, int sqr, size_t *out, bool crt)
{
    Plan P;
    const int rc = layout_out(make_plan_mod(&P, L, depth, w, sqr != 0, crt), P, out);
    if (!rc && crt) out[8] = P.off_lowd;
    return rc;
}

// d_b == d_a on a squaring plan
static int mod_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                      unsigned long w, bool sqr, void *d_ws, size_t ws_bytes, void *stream, bool crt)
{
    Plan P;
    int rc = make_plan_mod(&P, L, depth, w, sqr, crt);
    if (rc) return rc;
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    if (d_r == d_a || d_r == d_b) return MPFFT_EINVAL;
    return run_all_mod(P, d_r, d_a, d_b, (unsigned char *)d_ws, (hipStream_t)stream);
}

static int mod_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L, unsigned long depth,
                     unsigned long w, int sqr, void *d_ws, size_t ws_bytes, void *stream, bool crt)
{
    Plan P;
    int rc = make_plan_mod(&P, L, depth, w, sqr != 0, crt);
    if (rc) return rc;
    if ((stage & MPFFT_STAGE_DRIVEN) || stage == MPFFT_STAGE_FOLD_COMBINE) return MPFFT_EINVAL;
    if (stage == MPFFT_STAGE_LOWCONV && !crt) return MPFFT_EINVAL;
    if (stage != MPFFT_STAGE_FWD_COLUMNS && stage != MPFFT_STAGE_SCALE && stage != MPFFT_STAGE_COMBINE
        && stage != MPFFT_STAGE_LOWCONV)
        return single_stage(P, stage, d_a, sqr ? d_a : d_b, d_r, d_ws, ws_bytes, stream);   // the multiply's, Tr = NR
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    Exec X(P, (hipStream_t)stream);
    X.single((unsigned char *)d_ws);
    if (stage == MPFFT_STAGE_SCALE) return X.unweight();
    if (stage == MPFFT_STAGE_LOWCONV) return X.nlowconv(d_a, sqr ? d_a : d_b, (unsigned char *)d_ws);
    if (stage == MPFFT_STAGE_COMBINE)
        return crt ? X.ncombinew(d_r, (unsigned char *)d_ws) : X.ncombine(d_r, (unsigned char *)d_ws);
    if ((rc = X.nweight(d_a, sqr ? d_a : d_b, fwd_nops(P)))) return rc;
    return X.fwd_columns(nullptr, 0, nullptr, 0, fwd_nops(P), fwd_op(P));
}

static int mod_stage_kernels(long L, unsigned long depth, unsigned long w, int sqr, char *buf, size_t len, bool crt)
{
    Plan P;
    return stage_names_out(make_plan_mod(&P, L, depth, w, sqr != 0, crt), P, buf, len);
}

// fully reduced: the top limb 0, or 1 over L zero limbs
static bool mod_reduced(const uint64_t *a, long L)
{
    if (a[L] == 0) return true;
    if (a[L] != 1) return false;
    for (long i = 0; i < L; ++i)
        if (a[i]) return false;
    return true;
}

// Host operands of a product modulo 2^B + 1 (n = L + 1 limbs each) or 2^B - 1 (n = L) on the calling
// thread's device, as mul_host: io holds a, b and r; run(d_r, d_a, d_b, ws, stream) is the plan's driver
template <typename Run>
static int mod_host(const Plan &P, long n, uint64_t *r, const uint64_t *a, const uint64_t *b, Run run)
{
    int rc;
    HostCall H;
    const size_t nb = (size_t)n * 8;
    if ((rc = H.open(P.bytes, 3 * nb))) return rc;
    DevCtx &C = *H.C;
    u64 *d_a = C.io, *d_b = P.sqr ? d_a : d_a + n, *d_r = C.io + 2 * n;
    HIPCHK(hipMemcpyAsync(d_a, a, nb, hipMemcpyHostToDevice, C.stream));
    if (!P.sqr) HIPCHK(hipMemcpyAsync(d_b, b, nb, hipMemcpyHostToDevice, C.stream));
    if ((rc = run(d_r, d_a, d_b, C.ws, C.stream))) return rc;
    HIPCHK(hipMemcpyAsync(r, d_r, nb, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipStreamSynchronize(C.stream));
    g_last_ngpus = 1;
    return MPFFT_OK;
}

static int mod_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w,
                  bool sqr, bool crt)
{
    Plan P;
    int rc = make_plan_mod(&P, L, depth, w, sqr, crt);
    if (rc) return rc;
    if (!mod_reduced(a, L) || (!sqr && !mod_reduced(b, L))) return MPFFT_EINVAL;
    return mod_host(P, L + 1, r, a, b, [&](u64 *d_r, const u64 *d_a, const u64 *d_b, unsigned char *ws, hipStream_t s) {
        return run_all_mod(P, d_r, d_a, d_b, ws, s);
    });
}

// The *_choose and *_next_size of the mod 2^B + 1 families (make_plan_mod, with crt) and of mod 2^B - 1 (cyc:
// make_plan_cyc): mpfft_choose's candidates; a candidate's cost is choose_cost at its 2n slots, whatever L (on
// the low-word CRT family plus the convolution's 4 n^2 multiply-adds).
// fixed_L > 0: the candidates valid for that L; else each candidate at its smallest valid
// L >= min_L (a multiple of its granularity 2n / 64; crt: at least n limbs, bits1 >= 32)
static int mod_pick(long fixed_L, long min_L, long *L, unsigned long *depth, unsigned long *w, bool crt, bool cyc = false)
{
    Plan best;
    const bool found = search_grid(&best, [&](Plan *p, unsigned long d, unsigned long wv) {
        const long g = std::max<long>(1, (2L << d) / 64);
        long Lc = fixed_L > 0 ? fixed_L : (min_L + g - 1) / g * g;
        if (crt && fixed_L <= 0) Lc = std::max(Lc, 1L << d);
        return cyc ? make_plan_cyc(p, Lc, d, wv, CYC_MUL) : make_plan_mod(p, Lc, d, wv, false, crt);
    });
    if (!found) return crt && fixed_L > 0 && fixed_L < 4 ? MPFFT_EINVAL : MPFFT_ETOOBIG;   // L < 4: no bits1 >= 32
    *L = best.n1;
    *depth = (unsigned long)best.depth;
    *w = (unsigned long)best.w;
    return MPFFT_OK;
}

extern "C" {

int mpfft_mulmod_check_params(long L, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_mod(&P, L, depth, w, false);
}

size_t mpfft_mulmod_workspace_bytes(long L, unsigned long depth, unsigned long w, int sqr)
{
    return mod_workspace_bytes(L, depth, w, sqr, false);
}

int mpfft_mulmod_plan_info(long L, unsigned long depth, unsigned long w, long *out)
{
    return mod_plan_info(L, depth, w, out, false);
}

int mpfft_mulmod_workspace_layout(long L, unsigned long depth, unsigned long w, int sqr, size_t *out)
{
    return mod_workspace_layout(L, depth, w, sqr, out, false);
}

int mpfft_mulmod_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                        unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_device(d_r, d_a, d_b, L, depth, w, false, d_ws, ws_bytes, stream, false);
}

int mpfft_sqrmod_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                        void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_device(d_r, d_a, d_a, L, depth, w, true, d_ws, ws_bytes, stream, false);
}

int mpfft_mulmod_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                       unsigned long depth, unsigned long w, int sqr, void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_stage(stage, d_a, d_b, d_r, L, depth, w, sqr, d_ws, ws_bytes, stream, false);
}

int mpfft_mulmod_stage_kernels(long L, unsigned long depth, unsigned long w, int sqr, char *buf, size_t len)
{
    return mod_stage_kernels(L, depth, w, sqr, buf, len, false);
}

int mpfft_mulmod_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w)
{
    return mod_ex(r, a, b, L, depth, w, false, false);
}

int mpfft_sqrmod_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w)
{
    return mod_ex(r, a, a, L, depth, w, true, false);
}

int mpfft_mulmod_choose(long L, unsigned long *depth, unsigned long *w)
{
    long Lc = 0;
    if (L < 1) return MPFFT_EINVAL;
    return mod_pick(L, 0, &Lc, depth, w, false);
}

int mpfft_mulmod_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w)
{
    if (min_L < 1) return MPFFT_EINVAL;
    return mod_pick(0, min_L, L, depth, w, false);
}

// the low-word CRT family (MPFFT_VERSION 7)
int mpfft_mulmodw_check_params(long L, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_mod(&P, L, depth, w, false, true);
}

size_t mpfft_mulmodw_workspace_bytes(long L, unsigned long depth, unsigned long w, int sqr)
{
    return mod_workspace_bytes(L, depth, w, sqr, true);
}

int mpfft_mulmodw_plan_info(long L, unsigned long depth, unsigned long w, long *out)
{
    return mod_plan_info(L, depth, w, out, true);
}

int mpfft_mulmodw_workspace_layout(long L, unsigned long depth, unsigned long w, int sqr, size_t *out)
{
    return mod_workspace_layout(L, depth, w, sqr, out, true);
}

int mpfft_mulmodw_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                         unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_device(d_r, d_a, d_b, L, depth, w, false, d_ws, ws_bytes, stream, true);
}

int mpfft_sqrmodw_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                         void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_device(d_r, d_a, d_a, L, depth, w, true, d_ws, ws_bytes, stream, true);
}

int mpfft_mulmodw_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                        unsigned long depth, unsigned long w, int sqr, void *d_ws, size_t ws_bytes, void *stream)
{
    return mod_stage(stage, d_a, d_b, d_r, L, depth, w, sqr, d_ws, ws_bytes, stream, true);
}

int mpfft_mulmodw_stage_kernels(long L, unsigned long depth, unsigned long w, int sqr, char *buf, size_t len)
{
    return mod_stage_kernels(L, depth, w, sqr, buf, len, true);
}

int mpfft_mulmodw_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w)
{
    return mod_ex(r, a, b, L, depth, w, false, true);
}

int mpfft_sqrmodw_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w)
{
    return mod_ex(r, a, a, L, depth, w, true, true);
}

int mpfft_mulmodw_choose(long L, unsigned long *depth, unsigned long *w)
{
    long Lc = 0;
    if (L < 1) return MPFFT_EINVAL;
    return mod_pick(L, 0, &Lc, depth, w, true);
}

int mpfft_mulmodw_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w)
{
    if (min_L < 1) return MPFFT_EINVAL;
    return mod_pick(0, min_L, L, depth, w, true);
}

// ---- products mod 2^B - 1 (cyc.hpp, make_plan_cyc): run_all on a cyclic plan.  Out of scope as for
// the squares: the sqrt2 front end, the sharded and multi-GPU entries, mpfft_set_devices routing;
// the cached operand has no host handle. ---------------------------------------------------------
int mpfft_mulmodm1_check_params(long L, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_cyc(&P, L, depth, w, CYC_MUL);
}

size_t mpfft_mulmodm1_workspace_bytes(long L, unsigned long depth, unsigned long w, int kind)
{
    Plan P;
    return bytes_or_0(make_plan_cyc(&P, L, depth, w, kind), P);
}

int mpfft_mulmodm1_plan_info(long L, unsigned long depth, unsigned long w, long *out)
{
    Plan P;
    return plan_info_out(make_plan_cyc(&P, L, depth, w, CYC_MUL), P, out);
}

int mpfft_mulmodm1_workspace_layout(long L, unsigned long depth, unsigned long w, int kind, size_t *out)
{
    Plan P;
    return layout_out(make_plan_cyc(&P, L, depth, w, kind), P, out);
}

// [p, p + n) and [q, q + m) limbs share an address
static bool limbs_overlap(const uint64_t *p, long n, const uint64_t *q, long m) { return p < q + m && q < p + n; }

// d_b == d_a on a squaring plan and against the cached operand d_pre (kind CYC_PRE)
static int cyc_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth, unsigned long w,
                      int kind, void *d_ws, size_t ws_bytes, void *stream, const void *d_pre = nullptr, size_t pre_bytes = 0)
{
    Plan P;
    int rc = make_plan_cyc(&P, L, depth, w, kind);
    if (rc) return rc;
    if ((P.pre && !pre_ok(d_pre, pre_bytes, P)) || !ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    if (limbs_overlap(d_r, L, d_a, L) || limbs_overlap(d_r, L, d_b, L)) return MPFFT_EINVAL;
    return run_all(P, d_r, d_a, d_b, (unsigned char *)d_ws, (hipStream_t)stream, nullptr, (unsigned char *)d_pre);
}

int mpfft_mulmodm1_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                          unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    return cyc_device(d_r, d_a, d_b, L, depth, w, CYC_MUL, d_ws, ws_bytes, stream);
}

int mpfft_sqrmodm1_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                          void *d_ws, size_t ws_bytes, void *stream)
{
    return cyc_device(d_r, d_a, d_a, L, depth, w, CYC_SQR, d_ws, ws_bytes, stream);
}

int mpfft_mulmodm1_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                         unsigned long depth, unsigned long w, int kind, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    if (kind != CYC_MUL && kind != CYC_SQR) return MPFFT_EINVAL;
    int rc = make_plan_cyc(&P, L, depth, w, kind);
    if (rc) return rc;
    if ((stage & MPFFT_STAGE_DRIVEN) || stage == MPFFT_STAGE_FOLD_COMBINE) return MPFFT_EINVAL;
    if (stage != MPFFT_STAGE_SCALE && stage != MPFFT_STAGE_COMBINE)   // the multiply's, Tr = NR (the columns split)
        return single_stage(P, stage, d_a, kind == CYC_SQR ? d_a : d_b, d_r, d_ws, ws_bytes, stream);
    if (!ws_ok(d_ws, ws_bytes, P.bytes)) return MPFFT_ENOMEM;
    Exec X(P, (hipStream_t)stream);
    X.single((unsigned char *)d_ws);
    if (stage == MPFFT_STAGE_SCALE) return X.cscale();
    return X.ccombine(d_r, (unsigned char *)d_ws);
}

int mpfft_mulmodm1_stage_kernels(long L, unsigned long depth, unsigned long w, int kind, char *buf, size_t len)
{
    Plan P;
    return stage_names_out(make_plan_cyc(&P, L, depth, w, kind), P, buf, len);
}

// host operands: mod_host with L limbs each and the multiply's driver
static int cyc_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w, int kind)
{
    Plan P;
    int rc = make_plan_cyc(&P, L, depth, w, kind);
    if (rc) return rc;
    return mod_host(P, L, r, a, b, [&](u64 *d_r, const u64 *d_a, const u64 *d_b, unsigned char *ws, hipStream_t s) {
        return run_all(P, d_r, d_a, d_b, ws, s);
    });
}

int mpfft_mulmodm1_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w)
{
    return cyc_ex(r, a, b, L, depth, w, CYC_MUL);
}

int mpfft_sqrmodm1_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w)
{
    return cyc_ex(r, a, a, L, depth, w, CYC_SQR);
}

size_t mpfft_mulmodm1_precomp_bytes(long L, unsigned long depth, unsigned long w)
{
    Plan P;
    if (make_plan_cyc(&P, L, depth, w, CYC_MUL)) return 0;
    return plan_pre_bytes(P);
}

int mpfft_mulmodm1_precomp_device(void *d_pre, size_t pre_bytes, const uint64_t *d_b, long L, unsigned long depth,
                                  unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return device_run(make_plan_cyc(&P, L, depth, w, CYC_MUL), P, nullptr, nullptr, d_b, d_ws, ws_bytes, stream, d_pre,
                      pre_bytes, true);
}

int mpfft_mulmodm1_mul_precomp_device(uint64_t *d_r, const uint64_t *d_a, const void *d_pre, size_t pre_bytes, long L,
                                      unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    return cyc_device(d_r, d_a, d_a, L, depth, w, CYC_PRE, d_ws, ws_bytes, stream, d_pre, pre_bytes);
}

int mpfft_mulmodm1_choose(long L, unsigned long *depth, unsigned long *w)
{
    long Lc = 0;
    if (L < 1) return MPFFT_EINVAL;
    return mod_pick(L, 0, &Lc, depth, w, false, true);
}

int mpfft_mulmodm1_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w)
{
    if (min_L < 1) return MPFFT_EINVAL;
    return mod_pick(0, min_L, L, depth, w, false, true);
}

// ---- sums of products (mpfft_dot_*, MPFFT_VERSION 8) -----------------------------------------
int mpfft_dot_check_params(long K, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_dot(&P, K, n1, n2, depth, w);
}

int mpfft_dot_plan_info(long K, long n1, long n2, unsigned long depth, unsigned long w, long *out)
{
    Plan P;
    return plan_info_out(make_plan_dot(&P, K, n1, n2, depth, w), P, out);
}

size_t mpfft_dot_workspace_bytes(long K, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return bytes_or_0(make_plan_dot(&P, K, n1, n2, depth, w), P);
}

// out[11]: the multiply's eight words, then C's arrays
static int dot_layout_out(int rc, const Plan &P, size_t *out)
{
    if ((rc = layout_out(rc, P, out))) return rc;
    out[8] = P.off_digC; out[9] = P.off_topC; out[10] = P.off_cbC;
    return MPFFT_OK;
}

int mpfft_dot_workspace_layout(long K, long n1, long n2, unsigned long depth, unsigned long w, size_t *out)
{
    Plan P;
    return dot_layout_out(make_plan_dot(&P, K, n1, n2, depth, w), P, out);
}

int mpfft_dot_choose(long K, long n1, long n2, unsigned long *depth, unsigned long *w)
{
    if (K < 1 || K > DOT_MAX) return MPFFT_EINVAL;
    return choose_on_grid(depth, w, [&](Plan *p, unsigned long d, unsigned long wv) { return make_plan_dot(p, K, n1, n2, d, wv); });
}

// The device entry of the sums: signed (sd: the workspace is sd_layout's) and not (neg = 0, the dot plan's own)
static int dot_device(int rc, const Plan &P, bool sd, uint64_t *d_r, long K, u64 neg, const uint64_t *const *d_a,
                      const uint64_t *const *d_b, void *d_ws, size_t ws_bytes, void *stream)
{
    if (rc) return rc;
    if (!d_r || !d_a || !d_b) return MPFFT_EINVAL;
    if (!ws_ok(d_ws, ws_bytes, sd ? sd_layout(P).bytes : P.bytes)) return MPFFT_ENOMEM;
    return run_dot(P, K, d_r, (unsigned char *)d_ws, (hipStream_t)stream, [&](long i, const u64 **a, const u64 **b) {
        *a = d_a[i];
        *b = d_b[i];
        return *a && *b ? MPFFT_OK : MPFFT_EINVAL;
    }, neg);
}

int mpfft_dot_device(uint64_t *d_r, long K, const uint64_t *const *d_a, const uint64_t *const *d_b, long n1, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return dot_device(make_plan_dot(&P, K, n1, n2, depth, w), P, false, d_r, K, 0, d_a, d_b, d_ws, ws_bytes, stream);
}

// The pointwise field of a dot plan: what the first term runs + what the later terms run
int mpfft_dot_stage_kernels(long K, long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P;
    int rc = make_plan_dot(&P, K, n1, n2, depth, w);
    if (rc) return rc;
    std::string names = stage_kernel_names(P);
    size_t f0 = 0;   // the third of the seven ';'-joined fields
    for (int k = 0; k < 2; ++k) f0 = names.find(';', f0) + 1;
    const size_t f1 = names.find(';', f0);
    std::string pw = names.substr(f0, f1 - f0);
    if (pw_family(P) == PWF_NESTED) {
        std::string acc = pw;
        acc.replace(acc.find("k_pwss"), 6, "k_pwsa");
        pw += " + " + acc;
    } else {
        pw += " + k_slotacc";
    }
    names.replace(f0, f1 - f0, pw);
    return copy_out(names, buf, len);
}

int mpfft_dot_stage(int stage, long K, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1, long n2,
                    unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan_dot(&P, K, n1, n2, depth, w);
    if (rc) return rc;
    const bool acc = (stage & MPFFT_STAGE_ACC) != 0;
    stage &= ~MPFFT_STAGE_ACC;
    if (acc && stage != MPFFT_STAGE_POINTWISE) return MPFFT_EINVAL;
    if (!d_ws || ws_bytes < P.bytes) return MPFFT_ENOMEM;
    if (stage == MPFFT_STAGE_POINTWISE) {
        (void)hipGetLastError();
        Exec X(P, (hipStream_t)stream);
        X.single((unsigned char *)d_ws);
        if (acc) return X.pointwise_dot(true);
        if ((rc = X.pointwise_dot(false))) return rc;
        return X.copy_to_c();   // (no row level is fused here: the product was formed in place in A)
    }
    if (stage == MPFFT_STAGE_FWD_COLUMNS || stage == MPFFT_STAGE_FWD_ROWS)
        return single_stage(P, stage, d_a, d_b, d_r, d_ws, ws_bytes, stream);
    return single_stage(P, stage, d_a, d_b, d_r, d_ws, ws_bytes, stream, nullptr, true);   // the inverse side reads C
}

// Host operands: the context's io buffer holds one term's operands and, behind them, the sum; each
// term's copies are queued on the context's stream in front of its forward passes.
// neg: mpfft_sdot_ex's sign mask (the workspace then has sd_layout's regions behind the dot's; D lives
// there, so no operand is kept after its term)
// rc, P: the caller's make_plan_dot or make_plan_sdot
static int dot_host(int rc, const Plan &P, uint64_t *r, long K, u64 neg, const uint64_t *const *a, const uint64_t *const *b)
{
    if (rc) return rc;
    if (!r || !a || !b) return MPFFT_EINVAL;
    const long n1 = P.n1, n2 = P.n2;
    HostCall H;
    if ((rc = H.open(neg ? sd_layout(P).bytes : P.bytes, (size_t)(n1 + n2 + P.total) * 8))) return rc;
    u64 *d_a = H.C->io, *d_b = d_a + n1, *d_r = d_b + n2;
    hipStream_t s = H.C->stream;
    rc = run_dot(P, K, d_r, H.C->ws, s, [&](long i, const u64 **pa, const u64 **pb) {
        if (!a[i] || !b[i]) return (int)MPFFT_EINVAL;
        HIPCHK(hipMemcpyAsync(d_a, a[i], (size_t)n1 * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_b, b[i], (size_t)n2 * 8, hipMemcpyHostToDevice, s));
        *pa = d_a;
        *pb = d_b;
        return (int)MPFFT_OK;
    }, neg);
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    HIPCHK(hipMemcpyAsync(r, d_r, (size_t)P.total * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MPFFT_OK;
}

int mpfft_dot_ex(uint64_t *r, long K, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2,
                 unsigned long depth, unsigned long w)
{
    Plan P;
    return dot_host(make_plan_dot(&P, K, n1, n2, depth, w), P, r, K, 0, a, b);
}

int mpfft_dot_auto(uint64_t *r, long K, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2)
{
    unsigned long d = 0, wv = 0;
    const int rc = mpfft_dot_choose(K, n1, n2, &d, &wv);
    if (rc) return rc;
    return mpfft_dot_ex(r, K, a, b, n1, n2, d, wv);
}

// ---- small matrix products (mpfft_matmul_*, MPFFT_VERSION 10) -----------------------------------
int mpfft_matmul_check_params(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
}

size_t mpfft_matmul_workspace_bytes(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    if (make_plan_matmul(&P, m, k, p, n1, n2, depth, w)) return 0;
    return mm_layout(P, m, k, p).bytes;
}

int mpfft_matmul_workspace_layout(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w, size_t *out)
{
    Plan P;
    int rc = make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
    if (rc) return rc;
    if (!out) return MPFFT_EINVAL;
    if ((rc = dot_layout_out(rc, P, out))) return rc;
    const MmLayout L = mm_layout(P, m, k, p);
    out[11] = L.off_cache; out[12] = L.stride; out[13] = (size_t)L.ncache;
    return MPFFT_OK;
}

int mpfft_matmul_device(uint64_t *const *d_r, long m, long k, long p, const uint64_t *const *d_a, const uint64_t *const *d_b,
                        long n1, long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    int rc = make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
    if (rc) return rc;
    if (!d_r || !d_a || !d_b) return MPFFT_EINVAL;
    for (long e = 0; e < m * p; ++e)
        if (!d_r[e]) return MPFFT_EINVAL;
    for (long e = 0; e < m * k; ++e)
        if (!d_a[e]) return MPFFT_EINVAL;
    for (long e = 0; e < k * p; ++e)
        if (!d_b[e]) return MPFFT_EINVAL;
    if (!ws_ok(d_ws, ws_bytes, mm_layout(P, m, k, p).bytes)) return MPFFT_ENOMEM;
    return run_matmul(P, (int)m, (int)k, (int)p, (u64 *const *)d_r, (unsigned char *)d_ws, (hipStream_t)stream,
                      [&](int e, const u64 **d) {
                          *d = e < m * k ? d_a[e] : d_b[e - m * k];
                          return (int)MPFFT_OK;
                      });
}

// Host pointers: the context's io buffer holds one operand at a time (its copy is queued in front of
// its forward passes, on the same stream) and, behind it, the m p results
int mpfft_matmul_ex(uint64_t *const *r, long m, long k, long p, const uint64_t *const *a, const uint64_t *const *b, long n1,
                    long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    int rc = make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
    if (rc) return rc;
    if (!r || !a || !b) return MPFFT_EINVAL;
    for (long e = 0; e < m * p; ++e)
        if (!r[e]) return MPFFT_EINVAL;
    for (long e = 0; e < m * k; ++e)
        if (!a[e]) return MPFFT_EINVAL;
    for (long e = 0; e < k * p; ++e)
        if (!b[e]) return MPFFT_EINVAL;
    const long nin = n1 > n2 ? n1 : n2;
    HostCall H;
    if ((rc = H.open(mm_layout(P, m, k, p).bytes, (size_t)(nin + m * p * P.total) * 8))) return rc;
    u64 *d_in = H.C->io;
    hipStream_t s = H.C->stream;
    u64 *d_rs[MM_MAX * MM_MAX];
    for (long e = 0; e < m * p; ++e) d_rs[e] = d_in + nin + e * P.total;
    rc = run_matmul(P, (int)m, (int)k, (int)p, d_rs, H.C->ws, s, [&](int e, const u64 **d) {
        const bool isa = e < m * k;
        HIPCHK(hipMemcpyAsync(d_in, isa ? a[e] : b[e - m * k], (size_t)(isa ? n1 : n2) * 8, hipMemcpyHostToDevice, s));
        *d = d_in;
        return (int)MPFFT_OK;
    });
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    for (long e = 0; e < m * p; ++e)
        HIPCHK(hipMemcpyAsync(r[e], d_rs[e], (size_t)P.total * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MPFFT_OK;
}

int mpfft_matmul_auto(uint64_t *const *r, long m, long k, long p, const uint64_t *const *a, const uint64_t *const *b, long n1,
                      long n2)
{
    if (m < 1 || m > MM_MAX || k < 1 || k > MM_MAX || p < 1 || p > MM_MAX) return MPFFT_EINVAL;
    unsigned long d = 0, wv = 0;
    const int rc = mpfft_dot_choose(k, n1, n2, &d, &wv);
    if (rc) return rc;
    return mpfft_matmul_ex(r, m, k, p, a, b, n1, n2, d, wv);
}

// The dot plan's seven fields with the pointwise field replaced: what writes the caches + what forms a
// result entry's sum
int mpfft_matmul_stage_kernels(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w, char *buf,
                               size_t len)
{
    Plan P;
    int rc = make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
    if (rc) return rc;
    std::string names = stage_kernel_names(P);
    size_t f0 = 0;   // the third of the seven ';'-joined fields
    for (int i = 0; i < 2; ++i) f0 = names.find(';', f0) + 1;
    const size_t f1 = names.find(';', f0);
    std::string pw = names.substr(f0, f1 - f0);
    if (pw_family(P) == PWF_NESTED) {
        const int lk = pwss_lk_of(P.l), M = pw_inner_limbs(P.l, lk);
        char mm[96];
        snprintf(mm, sizeof mm, " + k_pwmm<%d> (single launch, K=%d)", M, 1 << lk);
        pw.replace(pw.find("k_pwss"), 6, "k_pwsx");   // the caches are written through that kernel's loaders
        pw += mm;
    } else {
        pw.insert(pw.size(), " (B cached) + k_slotacc");
    }
    names.replace(f0, f1 - f0, pw);
    return copy_out(names, buf, len);
}

int mpfft_matmul_stage(int stage, long m, long k, long p, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1,
                       long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream, long kk,
                       const int *ea, const int *eb)
{
    Plan P;
    int rc = make_plan_matmul(&P, m, k, p, n1, n2, depth, w);
    if (rc) return rc;
    const bool acc = (stage & MPFFT_STAGE_ACC) != 0;
    const int st = stage & ~MPFFT_STAGE_ACC;
    if (st != MPFFT_STAGE_MM_STORE && st != MPFFT_STAGE_MM_POINTWISE)   // the dot workspace sits at the front
        return mpfft_dot_stage(stage, k, d_a, d_b, d_r, n1, n2, depth, w, d_ws, ws_bytes, stream);
    const MmLayout L = mm_layout(P, m, k, p);
    if (!ea || (acc && st != MPFFT_STAGE_MM_POINTWISE)) return MPFFT_EINVAL;
    if (!ws_ok(d_ws, ws_bytes, L.bytes)) return MPFFT_ENOMEM;
    unsigned char *ws = (unsigned char *)d_ws;
    Exec X(P, (hipStream_t)stream);
    X.single(ws);
    X.pre_make = true;   // (like mpfft_dot_stage it never fuses row levels)
    if (st == MPFFT_STAGE_MM_STORE) {
        if (ea[0] < 0 || ea[0] >= L.ncache) return MPFFT_EINVAL;
        X.pre = ws + L.off_cache + (size_t)ea[0] * L.stride;
        return X.precomp_store(ea[0] < m * k ? 0 : 1);
    }
    if (!eb || kk < 1 || kk > MM_MAX) return MPFFT_EINVAL;
    for (long i = 0; i < kk; ++i)
        if (ea[i] < 0 || ea[i] >= L.ncache || eb[i] < 0 || eb[i] >= L.ncache) return MPFFT_EINVAL;
    return X.pointwise_mm(ws + L.off_cache, L.stride, (int)kk, ea, eb, acc);
}

// ---- signed sums of products (mpfft_sdot_*, MPFFT_VERSION 9; sdot.hpp) -------------------------
// the dot plan; MPFFT_EINVAL for a mask bit at or above K
static int make_plan_sdot(Plan *p, long K, u64 neg, long n1, long n2, unsigned long depth, unsigned long w)
{
    const int rc = make_plan_dot(p, K, n1, n2, depth, w);
    if (rc) return rc;
    return K < 64 && (neg >> K) ? MPFFT_EINVAL : MPFFT_OK;
}

int mpfft_sdot_check_params(long K, uint64_t neg, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    return make_plan_sdot(&P, K, neg, n1, n2, depth, w);
}

size_t mpfft_sdot_workspace_bytes(long K, long n1, long n2, unsigned long depth, unsigned long w)
{
    Plan P;
    if (make_plan_dot(&P, K, n1, n2, depth, w)) return 0;
    return sd_layout(P).bytes;
}

int mpfft_sdot_workspace_layout(long K, long n1, long n2, unsigned long depth, unsigned long w, size_t *out)
{
    Plan P;
    const int rc = dot_layout_out(make_plan_dot(&P, K, n1, n2, depth, w), P, out);
    if (rc) return rc;
    const SdLayout L = sd_layout(P);
    out[11] = L.off_scr;
    out[12] = L.off_d;
    return MPFFT_OK;
}

int mpfft_sdot_device(uint64_t *d_r, long K, uint64_t neg, const uint64_t *const *d_a, const uint64_t *const *d_b, long n1,
                      long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    return dot_device(make_plan_sdot(&P, K, neg, n1, n2, depth, w), P, true, d_r, K, neg, d_a, d_b, d_ws, ws_bytes, stream);
}

int mpfft_sdot_ex(uint64_t *r, long K, uint64_t neg, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2,
                  unsigned long depth, unsigned long w)
{
    Plan P;
    return dot_host(make_plan_sdot(&P, K, neg, n1, n2, depth, w), P, r, K, neg, a, b);
}

int mpfft_sdot_auto(uint64_t *r, long K, uint64_t neg, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2)
{
    unsigned long d = 0, wv = 0;
    if (K >= 1 && K < 64 && (neg >> K)) return MPFFT_EINVAL;
    const int rc = mpfft_dot_choose(K, n1, n2, &d, &wv);
    if (rc) return rc;
    return mpfft_sdot_ex(r, K, neg, a, b, n1, n2, d, wv);
}

// The dot's seven fields; with a negative term the pre-pass in front of the forward columns' and the
// correction behind the combine's
int mpfft_sdot_stage_kernels(long K, uint64_t neg, long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len)
{
    Plan P;
    int rc = make_plan_sdot(&P, K, neg, n1, n2, depth, w);
    if (rc) return rc;
    if (!buf || !len) return MPFFT_EINVAL;
    std::vector<char> tmp(len);
    if ((rc = mpfft_dot_stage_kernels(K, n1, n2, depth, w, tmp.data(), len))) return rc;
    std::string names = tmp.data();
    if (neg) names = "k_sdneg + " + names + " + k_sdedge + k_sdfix (blocks of 4096 limbs)";
    return copy_out(names, buf, len);
}

int mpfft_sdot_stage(int stage, long K, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan P;
    const int rc = make_plan_dot(&P, K, n1, n2, depth, w);
    if (rc) return rc;
    const int st = stage & ~MPFFT_STAGE_ACC;
    const bool acc = (stage & MPFFT_STAGE_ACC) != 0;
    if (acc && st != MPFFT_STAGE_SD_NEG && st != MPFFT_STAGE_POINTWISE) return MPFFT_EINVAL;
    if (!d_ws || ws_bytes < sd_layout(P).bytes) return MPFFT_ENOMEM;
    if (st != MPFFT_STAGE_SD_NEG && st != MPFFT_STAGE_SD_FIX)   // the dot workspace at the front of this one
        return mpfft_dot_stage(stage, K, d_a, d_b, d_r, n1, n2, depth, w, d_ws, ws_bytes, stream);
    (void)hipGetLastError();
    Exec X(P, (hipStream_t)stream);
    X.single((unsigned char *)d_ws);
    if (st == MPFFT_STAGE_SD_NEG) return d_a && d_b ? X.sd_neg(d_a, d_b, (unsigned char *)d_ws, !acc) : MPFFT_EINVAL;
    return d_r ? X.sd_fix(d_r, (unsigned char *)d_ws) : MPFFT_EINVAL;
}

// release the calling device's cached workspace (the next call re-allocates)
int mpfft_release(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MPFFT_MAX_DEV) return MPFFT_ENODEV;
    DevCtx &C = g_dev[dev];
    std::lock_guard<std::mutex> lk(C.mu);
    if (C.ws) (void)hipFree(C.ws);
    if (C.io) (void)hipFree(C.io);
    C.ws = nullptr;
    C.io = nullptr;
    C.ws_bytes = C.io_bytes = 0;
    return MPFFT_OK;
}

int mpfft_choose(long n1, long n2, unsigned long *depth, unsigned long *w)
{
    return choose_on_grid(depth, w, [&](Plan *p, unsigned long d, unsigned long wv) { return make_plan(p, n1, n2, d, wv); });
}

int mpfft_mul_auto(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2)
{
    unsigned long d = 0, wv = 0;
    const int rc = mpfft_choose(n1, n2, &d, &wv);
    if (rc) return rc;
    return mpfft_mul_ex(r1, i1, n1, i2, n2, d, wv);
}

int mpfft_sqr_auto(uint64_t *r, const uint64_t *a, long n)
{
    unsigned long d = 0, wv = 0;
    const int rc = mpfft_choose(n, n, &d, &wv);
    if (rc) return rc;
    return mpfft_sqr_ex(r, a, n, d, wv);
}

// mul_fft.c:3190 -- same signature and meaning; fails loudly instead of segfaulting
void new_mpn_mul(mp_limb_t *r1, mp_limb_t *i1, mp_size_t n1, mp_limb_t *i2, mp_size_t n2, mp_bitcnt_t depth,
                 mp_bitcnt_t w)
{
    die_on(mpfft_mul_ex(r1, i1, n1, i2, n2, depth, w), "new_mpn_mul", (long)n1, (long)n2, depth, w);
}

// splitmix64-seeded xoshiro256** (BASELINE.md synthetic inputs; same stream as the oracle's)
void mpfft_fill_random(uint64_t *buf, long cnt, uint64_t seed)
{
    uint64_t s[4], z = seed;
    for (int i = 0; i < 4; i++) {
        z += 0x9e3779b97f4a7c15ULL;
        uint64_t x = z;
        x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
        x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
        s[i] = x ^ (x >> 31);
    }
    for (long i = 0; i < cnt; i++) {
        const uint64_t r = s[1] * 5;
        buf[i] = ((r << 7) | (r >> 57)) * 9;
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t;
        s[3] = (s[3] << 45) | (s[3] >> 19);
    }
}

}  // extern "C"
