// plan.hpp -- everything new_mpn_mul decides without touching a device: the parameters and
// workspace layout of one product (Plan), the pointwise kernel family and the (depth, w)
// chooser's cost model.  Included by mpfft.hip only, after the kernel and dispatch headers.
#pragma once

// ---------------------------------------------------------------------------
// parameters (mul_fft.c:3193-3203)
// ---------------------------------------------------------------------------
// Tuning / ablation / stamp knobs exist only in a diagnostic build (make DIAG=1 defines
// MPFFT_DIAG); the shipped library never reads them, so no environment can make it skip
// work or run an untested kernel family.
static const char *diag_env(const char *name)
{
#ifdef MPFFT_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// wave kernels for coefficients of l limbs: U = ceil(l / 64) limbs per lane, full rows when l == 64 U
// (here, not with the other dispatch in exec.hpp: the plan takes their maxlogg)
static WvFns wv_fns(int U, bool full)
{
    switch (U) {
    case 1: return full ? wv_fns_u1_1() : wv_fns_u1_0();
    case 2: return full ? wv_fns_u2_1() : wv_fns_u2_0();
    case 3: return full ? wv_fns_u3_1() : wv_fns_u3_0();
    default: return full ? wv_fns_u4_1() : wv_fns_u4_0();
    }
}

struct Plan {
    long n1, n2;
    int depth;
    long w;
    long n, l;
    u64 N, bits1;
    long NC, NR;
    int lbC, lbR;
    long j1, j2, trunc, Tr, len, total;
    int U, tpb, maxlogg;
    int maxlogg_c;      // column passes (forward and inverse); maxlogg: row passes
    int maxlogg_i;      // inverse (DIT) k_rpass passes, rows and columns (0: as above)
    int bp_lg;          // most levels k_bpass fits in LDS (big): a pass k_rpass declines is capped to it
    bool wave;          // wave-owned coefficient kernels (wkernels.hpp), l <= 512
    int wU;             // their limbs per lane
    bool wfull;         // l == 64 wU
    bool fuse_scale;    // scaling fused into the last inverse column pass (no truncation)
    bool lds;           // LDS-resident radix-2^5 passes (lkernels.hpp)
    bool big;           // LDS-resident passes for 512 <= l <= 4096 (bkernels.hpp)
    bool rpass;         // register-resident passes (rkernels.hpp) where they apply, l = 1024, 2048, 4096
    bool sqrt2;         // new_mpn_mul6 plan: 4n slots, bits1 = (N - depth - 1)/2, Tr up to 2 NR
    size_t slots;       // allocated slots per operand
    // off_flags: k_combine1's look-back flags + ticket counter, cleared by the first forward
    // column pass
    // (Exec::zflags) -- no stage between that pass and the combine may use this region
    size_t off_digA, off_topA, off_cbA, off_digB, off_topB, off_cbB, off_flags, bytes;
    bool has_c;         // a third coefficient array C: the fused pointwise (k_pwss PAIR) writes there
    int fold;           // f4 (fold.hpp): scaling in the last inverse row pass, reduced-form combine with
                        // KM = fold coefficients per wave (0: k_rscale + k_combine1)
    bool ltw;           // fold plans: the inverse MFA twiddle and the scaling ride in the first pass of
                        // each column block of the truncated inverse (k_rpass DIT mode bit 3) instead
                        // of the rows' last pass (every block's rotation a whole number of limb pairs)
    size_t off_meta;    // k_cmeta's per-coefficient A_k, B_k (fold plans)
    int fuse_rows;      // row DIF levels that run inside the pointwise: 1 (slot pairs), 2 (slot quads), 0
    size_t off_digC, off_topC, off_cbC;
    bool sqr;           // squaring plan (make_plan_sqr): one operand, no B arrays in the layout
    bool pre;           // multiply against a precomputed operand B (make_plan_pre): no B arrays in the layout
                        // either, but two operands -- the pointwise reads B from the cache (plan_pre_bytes)
    // make_plan_mod: a product mod 2^(64 n1) + 1 as a length-2n negacyclic convolution (nega.hpp)
    bool nega;
    size_t off_nflags;  // k_nwrap's look-back flags, ticket counter and overflow word (behind off_flags:
                        // the weight launch clears both in one range)
    size_t off_nscr;    // the unsigned sum of the canonical coefficients (k_combine1's output), `total` limbs
    // make_plan_mod with crt (negaw.hpp): pieces up to the low-word CRT's bound; off_lowd: the low-word
    // convolution d, 2n u32, behind every region of the plain negacyclic plan
    bool lowcrt;
    size_t off_lowd;
    // make_plan_cyc: a product mod 2^(64 n1) - 1 as a length-2n cyclic convolution (cyc.hpp); off_nflags
    // and off_nscr hold k_cwrap's flags and the scratch sum as they do k_nwrap's on a negacyclic plan
    bool cyc;
};

static int ilog2(long v) { int d = 0; while ((1L << d) < v) ++d; return d; }

// pointwise kernel family.  MPFFT_POINTWISE is the one runtime selector the shipped library
// reads (every choice is an exact product; the parity tests A/B them): auto (default),
// pwss = the nested negacyclic k_pwss (l = 1024, 2048, 4096), mfma = int8-MFMA k_pwm2
// (l % 256 == 0), mfma1 = k_pwm (l % 128 == 0), valu = k_pw.
enum { PW_AUTO = 0, PW_PWSS, PW_MFMA, PW_MFMA1, PW_VALU };
static int pw_kind()
{
    const char *e = getenv("MPFFT_POINTWISE");
    if (!e) return PW_AUTO;
    if (!strcmp(e, "pwss")) return PW_PWSS;
    if (!strcmp(e, "mfma")) return PW_MFMA;
    if (!strcmp(e, "mfma1")) return PW_MFMA1;
    if (!strcmp(e, "valu")) return PW_VALU;
    return PW_AUTO;
}

// nested negacyclic pointwise (pkernels.hpp) for big coefficients: log2 of its piece count
// (0: another kernel).  Default from l = 2048 on; at l = 1024 the int8-MFMA schoolbook wins.
static int pwss_lk_of(long l)
{
    const int k = pw_kind();
    if (k != PW_AUTO && k != PW_PWSS) return 0;
    switch (l) {
    case 1024: return k != PW_AUTO ? 8 : 0;
    case 2048: return 8;
    case 4096: return 9;   // K = 1024 (M = 16, 1024 threads, 4 waves/SIMD) measured slower: C4 63.3 vs 45.3 ms
    }
    return 0;
}

// the fused-pair k_pwss instance (last row DIF level on load, product to C) exists for l;
// fuse 2: the fused-quad instance (the last two levels)
static bool pw_pair_kernel(long l, int fuse = 1)
{
    const int lk = pwss_lk_of(l);
    return lk && pw_get(pw_inner_limbs(l, lk), lk, fuse) != nullptr;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The pointwise kernel family of a plan, decided here alone: Exec::pointwise() launches it and
// the stage-kernel names print it.
enum PwFamily {
    PWF_NESTED,      // k_pwss / k_pwsq: nested negacyclic (pkernels.hpp)
    PWF_PWM2,        // k_pwm2: int8 MFMA, register-blocked: 2 fold tiles per wave
    PWF_PWM,         // k_pwm: int8 MFMA Toeplitz product
    PWF_PW,          // k_pw: register-blocked VALU kernel, R columns per thread
    PWF_POINTWISE    // k_pointwise: VALU
};
static PwFamily pw_family(const Plan &P)
{
    const int lk = pwss_lk_of(P.l), kind = pw_kind();
    if (lk && pw_get(pw_inner_limbs(P.l, lk), lk)) return PWF_NESTED;
    static const long pwm2_maxl = [] { const char *e = diag_env("MPFFT_PWM2_MAXL"); return e ? atol(e) : 4096L; }();
    if (P.l % 256 == 0 && P.l <= pwm2_maxl && kind != PW_MFMA1 && kind != PW_VALU) return PWF_PWM2;
    if (P.l % 128 == 0 && kind != PW_VALU) return PWF_PWM;
    if (P.l % 2 == 0 && P.l >= 32) return PWF_PW;
    return PWF_POINTWISE;
}

// sqrt2: the new_mpn_mul6 front end (mul_fft.c:3573-3603): a length-4n convolution with
// bits1 = (N - (depth + 1))/2 (:3578) and the same trunc rule (:3603)
// lbc >= 0: NC = 2^lbc instead of the reference's split; fwd4: four-level forward k_rpass passes
// sbits: bits of headroom the coefficients keep for a sum of up to 2^sbits products (make_plan_dot)
static int make_plan_split(Plan *p, long n1, long n2, unsigned long depth, unsigned long w, bool sqrt2, int lbc,
                           bool fwd4 = false, int sbits = 0)
{
    memset(p, 0, sizeof(*p));
    p->sqrt2 = sqrt2;
    if (n1 < 1 || n2 < 1) return MPFFT_EINVAL;
    if (depth < 2 || depth > 30 || w < 1 || w > 4096) return MPFFT_EINVAL;
    p->n1 = n1;
    p->n2 = n2;
    p->depth = (int)depth;
    p->w = (long)w;
    p->n = 1L << depth;
    if (((u64)p->n * w) % 64) return MPFFT_EINVAL;          // N must be a whole number of limbs
    p->N = (u64)p->n * w;
    p->l = (long)(p->N / 64);
    if (p->N <= depth) return MPFFT_EINVAL;
    if (sqrt2 && p->N <= depth + 1) return MPFFT_EINVAL;
    if (p->N <= depth + (u64)sbits) return MPFFT_EINVAL;
    p->bits1 = (p->N - depth - (sqrt2 ? 1 : 0) - (u64)sbits) / 2;
    if (p->bits1 < 1) return MPFFT_EINVAL;
    p->NC = 1L << (lbc >= 0 ? lbc : (int)depth / 2);   // the reference's split (mul_fft.c:3195) unless make_plan picks another
    p->NR = 2 * p->n / p->NC;
    p->lbC = ilog2(p->NC);
    p->lbR = ilog2(p->NR);
    p->j1 = (long)((64 * (u64)n1 - 1) / p->bits1 + 1);
    p->j2 = (long)((64 * (u64)n2 - 1) / p->bits1 + 1);
    p->len = p->j1 + p->j2 - 1;
    if (p->len > (sqrt2 ? 4 : 2) * p->n) return MPFFT_ETOOBIG;   // product does not fit the convolution
    p->trunc = ((p->j1 + p->j2 - 2 + 2 * p->NC) / (2 * p->NC)) * 2 * p->NC;
    p->Tr = p->trunc / p->NC;
    p->total = n1 + n2;
    if (p->l > 4096) return MPFFT_EUNSUPPORTED;              // pointwise LDS budget (24 l bytes)
    // threads per coefficient and limbs per thread: U == 1 kernels are built for
    // <= 256 threads (MPF_LB), U == 2 / 4 for <= 1024
    const int Up = p->l <= 256 ? 1 : p->l <= 2048 ? 2 : 4;
    long tpb = 64;
    while (tpb * Up < p->l) tpb *= 2;
    p->tpb = (int)tpb;
    p->U = Up;
    p->maxlogg = Up == 1 ? 4 : Up == 2 ? 2 : 1;   // G*U <= 8 keeps U >= 2 passes spill-free
    {
        const char *e = diag_env("MPFFT_WAVE");
        p->wave = p->l <= 256 && !(e && !strcmp(e, "0"));
    }
    if (p->wave) {
        p->wU = (int)((p->l + 63) / 64);
        p->wfull = p->l == 64L * p->wU;
        p->maxlogg = wv_fns(p->wU, p->wfull).maxlogg;
        const char *e = diag_env("MPFFT_WLOGG");
        if (e && atoi(e) >= 1 && atoi(e) <= p->maxlogg) p->maxlogg = atoi(e);
        p->fuse_scale = p->Tr == p->NR && !sqrt2;
        const char *el = diag_env("MPFFT_LDS");
        p->lds = !(el && !strcmp(el, "0"));
        if (p->lds) {
            p->maxlogg = LP_MAXLOGG;
            if (e && atoi(e) >= 1 && atoi(e) <= LP_MAXLOGG) p->maxlogg = atoi(e);
        }
    }
    {
        const char *e = diag_env("MPFFT_BIG");
        const long rows = p->l / 64;
        p->big = !p->wave && p->l >= 512 && p->l % 64 == 0 && !(rows & (rows - 1)) && !(e && !strcmp(e, "0"));
    }
    if (p->big) {   // as many levels per pass as coefficients fit in LDS (G <= 16)
        int lg = 1;
        while (lg < BP_MAXLOGG && bp_lds_need(p->l, 2 << lg) <= BP_LDS_MAX) ++lg;
        p->maxlogg = lg;
        p->bp_lg = lg;
        // columns: two 74 KB groups per CU beat one 147 KB group at l = 2048 (C3 sweep,
        // profiles/r02/sweep_blogg.txt: columns 5.97 ms vs 6.53 ms; rows 4.71 vs 4.44)
        p->maxlogg_c = lg >= 3 ? lg - 1 : lg;
        const char *e = diag_env("MPFFT_BLOGG");
        if (e && atoi(e) >= 1 && atoi(e) <= lg) p->maxlogg = p->maxlogg_c = atoi(e);
        const char *er = diag_env("MPFFT_RPASS");
        p->rpass = rp_maxlogg((int)p->l) > 0 && !(er && !strcmp(er, "0")) && !diag_env("MPFFT_BP_STAMPS");
        if (p->rpass && !e) {   // same levels per pass for columns and rows (two groups per CU either way)
            int rl = fwd4 ? rp_maxlogg_fwd4((int)p->l) : rp_maxlogg((int)p->l);   // register-resident: not bound by k_bpass's LDS fit
            const char *ec = diag_env("MPFFT_RPLOGG");   // diagnostics: fewer levels per pass (A/B)
            if (ec && atoi(ec) >= 1 && atoi(ec) < rl) rl = atoi(ec);
            p->maxlogg = p->maxlogg_c = rl;
            int ri = rp_maxlogg_dit((int)p->l);
            const char *ei = diag_env("MPFFT_RPLOGG_INV");
            if (ei && atoi(ei) >= 1 && atoi(ei) < ri) ri = atoi(ei);
            if (ec && rl < ri) ri = rl;
            p->maxlogg_i = ri;
        }
    }
    p->slots = (size_t)(sqrt2 ? 4 : 2) * p->n;
    size_t o = 0;
    const size_t dig = p->slots * p->l * 8, top = align_up(p->slots * 4, 256);
    const size_t cbb = align_up(p->slots * cb_words((int)p->l) * 8, 256);
    p->off_digA = o; o += dig;
    p->off_topA = o; o += top;
    p->off_cbA = o; o += cbb;
    p->off_digB = o; o += dig;
    p->off_topB = o; o += top;
    p->off_cbB = o; o += cbb;
    // C: output of the fused last-row-level pointwise (single-GPU new_mpn_mul, Exec::row_fused)
    // (only where it saves a row pass: fewer passes for lbC - 1 levels than for lbC)
    {
        // the last two levels where that saves a pass and one does not (C4: 8 row levels at <= 3
        // per pass are 3 + 3 + 2, 6 are 3 + 3); the quad form needs the plain MFA row root (not
        // the sqrt2 front end's)
        const int ml = p->maxlogg > 0 ? p->maxlogg : 1;
        auto np = [&](int L) { return (L + ml - 1) / ml; };
        const bool f1 = p->lbC >= 2 && np(p->lbC - 1) < np(p->lbC) && pw_pair_kernel(p->l);
        static const bool no2 = diag_env("MPFFT_NO_FUSE2") != nullptr;   // diagnostics: A/B
        const int lk = pwss_lk_of(p->l);   // quad inputs are 4x the pieces: 2 more bits of headroom (pdispatch.hpp)
        const bool room = lk && 64 * pw_inner_limbs(p->l, lk) >= 2 * ((64 * p->l) >> lk) + lk + 6;
        // ... or where it turns four-level row passes into three-level ones (8 row levels: 4 + 4 ->
        // fused 2 + 3 + 3 -- three-level passes run two workgroups per CU; C3 8.64 -> 8.55 ms,
        // profiles/r04/quad_fuse_ab.txt)
        const bool saves2 = np(p->lbC - 2) < np(p->lbC - 1) && np(p->lbC - 2) < np(p->lbC);
        const bool to3 = ml == 4 && p->lbC - 2 == 6;
        const bool f2 = !sqrt2 && !no2 && room && p->lbC >= 3 && (saves2 || to3) && pw_pair_kernel(p->l, 2);
        static const bool force2 = diag_env("MPFFT_FORCE_FUSE2") != nullptr;   // diagnostics: A/B
        const bool f2f = force2 && !sqrt2 && room && p->lbC >= 3 && pw_pair_kernel(p->l, 2);
        p->fuse_rows = (f2 || f2f) ? 2 : f1 ? 1 : 0;
        p->has_c = p->fuse_rows > 0;
    }
    if (p->has_c) {
        p->off_digC = o; o += dig;
        p->off_topC = o; o += top;
        p->off_cbC = o; o += cbb;
    }
    p->off_flags = o; o += align_up((size_t)(p->total / 256 + 8) * 4, 256);   // k_combine1 blocks at V = 1
    // f4 fold (fold.hpp) on the truncated register-pass plans: KM coefficients reach a wave's 512
    // product limbs (windows shifted by up to one bit); MPFFT_FOLD=0 (diagnostics): k_rscale + k_combine1
    {
        static const bool no_fold = [] { const char *e = diag_env("MPFFT_FOLD"); return e && !strcmp(e, "0"); }();
        const int km = (int)((p->N + 1 + 32767) / p->bits1 + 1);
        p->fold = (p->rpass && !sqrt2 && p->Tr < p->NR && p->bits1 > 512 && km <= 4 && !no_fold) ? (km <= 3 ? 3 : 4) : 0;
        static const bool no_ltw = [] { const char *e = diag_env("MPFFT_LTW"); return e && !strcmp(e, "0"); }();
        // where it measured faster: l <= 2048 (C3 inverse rows + columns 1.714 -> 1.679 ms); at
        // l = 4096 the rotated loads in the three-level column passes cost more than the rows save
        // (C4 15.54 -> 15.84 ms), profiles/r06/ltw_ab.txt
        p->ltw = p->fold && ((u64)p->w * (u64)p->NC) % 128 == 0 && p->l <= 2048 && !no_ltw;
    }
    p->off_meta = o; o += align_up((size_t)p->slots * 4, 256);
    p->bytes = o;
    return MPFFT_OK;
}

// rows of the truncated inverse column transform whose top-level doubling Exec::itft leaves to
// the scaling (defer_double): IFFT_radix2_truncate's t <= h branch doubles outputs [0, t), the
// t > h branch [t - h, h) (mul_fft.c:1733-1790)
static void plan_dbl(const Plan &P, long *lo, long *hi)
{
    const long t = P.Tr, h = P.NR / 2;
    *lo = *hi = 0;
    if (t == P.NR) return;
    if (t <= h) *hi = t;
    else {
        *lo = t - h;
        *hi = h;
    }
}

// The matrix split of the MFA is internal (no internal ABI): the reference takes
// NC = 2^floor(depth/2) columns (mul_fft.c:3195).  At l = 2048 with truncation case b
// (trunc > half the convolution), and since round 6 in case a at depth 13-15 as well (below),
// twice the columns with four-level forward passes is faster:
// C3 (depth 15) 256 x 256 runs its 8 column levels in 4 + 4 where 128 x 512 needs 3 + 3 + 3,
// 8.64 vs 8.81 ms; in case a the reference split's column transform skips its empty upper
// half and wins (C2: 6.69 vs 6.99 ms); at l = 4096 (C4) 512 x 512 with three-level passes
// measured slower (97.1 vs 96.2 ms).  profiles/r04/mfa_split_ab.txt.  Both splits give the
// same exact product.
static int make_plan(Plan *p, long n1, long n2, unsigned long depth, unsigned long w, bool sqrt2 = false, int sbits = 0)
{
    int rc = make_plan_split(p, n1, n2, depth, w, sqrt2, -1, false, sbits);
    // diagnostics (A/B): MPFFT_SPLIT=ref / alt forces a split
    static const char *force = diag_env("MPFFT_SPLIT");
    // l = 4096, truncation case b: twice the reference's columns since the live-group launches (C4 74.1-74.3
    // -> 72.2 ms, profiles/r06/c4_split_ab.txt; round 4, before them, measured it slower); case a unmeasured
    if (!rc && !sqrt2 && p->rpass && p->l == 4096 && !(force && !strcmp(force, "ref"))
        && (2 * p->Tr > p->NR || (force && !strcmp(force, "alt4")))) {
        Plan q;
        if (make_plan_split(&q, n1, n2, depth, w, sqrt2, (int)depth / 2 + 1, false, sbits) == MPFFT_OK && q.rpass) *p = q;
        return rc;
    }
    if (rc || sqrt2 || !p->rpass || p->l != 2048 || (force && !strcmp(force, "ref"))) return rc;
    // case a (2 Tr <= NR) too at depth 13-15 since the live-group launches (C2 6.09 -> 5.95 ms, -2.2 to
    // -4.8 % over truncation ratios 0.40-0.48 at depth 13-15, +0.3-0.5 % at depth 16:
    // profiles/r06/split_resweep.txt); smaller depths were not re-measured and keep the rule
    const bool casea = 2 * p->Tr <= p->NR;
    if (!(force && !strcmp(force, "alt")) && casea && (depth < 13 || depth > 15)) return rc;
    Plan q;
    if (make_plan_split(&q, n1, n2, depth, w, sqrt2, (int)depth / 2 + 1, true, sbits) == MPFFT_OK && q.rpass
        && (!casea || (force && !strcmp(force, "alt")) || q.trunc <= p->trunc + p->trunc / 64))   // case a: at most 1/64 more truncated length
        *p = q;
    return MPFFT_OK;
}

// operand B's arrays (dig + top + cbb of make_plan_split) out of a plan's layout: everything
// behind them moves down by their size.  sqr: a squaring plan; else a multiply against a
// precomputed operand (Plan::pre)
static void plan_drop_b(Plan *p, bool sqr = true)
{
    const size_t b = (p->has_c ? p->off_digC : p->off_flags) - p->off_digB;
    p->sqr = sqr;
    p->pre = !sqr;
    p->off_digB = p->off_topB = p->off_cbB = 0;
    if (p->has_c) {
        p->off_digC -= b;
        p->off_topC -= b;
        p->off_cbC -= b;
    }
    p->off_flags -= b;
    p->off_meta -= b;
    p->bytes -= b;
}

// Sum of K products (mpfft_dot_*): r = sum_{i < K} a_i b_i, every a_i of n1 and every b_i of n2 limbs.
// The multiply's planner with bits1 = (N - depth - s) / 2, s = ceil(log2 K): a coefficient of the summed
// convolutions is c_k <= K min(j1, j2) (2^bits1 - 1)^2 < 2^(s + depth + 2 bits1) <= 2^N (min(j1, j2) <=
// n = 2^depth since j1 + j2 - 1 <= 2n), so the sum is read off the residues mod 2^N + 1 as one product
// is -- the multiply's own bits1 leaves no such room when N - depth is even.  j1, j2, trunc, the split,
// fold, ltw and fuse_rows follow from that bits1 as the multiply's do.  The sum has n1 + n2 + 1 limbs
// (the top one below K), and every dot plan has the C arrays: the accumulator.  K = 1 is the
// multiply's plan apart from those two.
static const int DOT_MAX = 64;
static int dot_sbits(long K) { return ilog2(K); }
static int make_plan_dot(Plan *p, long K, long n1, long n2, unsigned long depth, unsigned long w)
{
    if (K < 1 || K > DOT_MAX) {
        memset(p, 0, sizeof(*p));
        return MPFFT_EINVAL;
    }
    const int rc = make_plan(p, n1, n2, depth, w, false, dot_sbits(K));
    if (rc) return rc;
    p->total = n1 + n2 + 1;
    // the regions behind B again: C, the combine flags for `total` limbs, the fold's meta words
    size_t o = p->has_c ? p->off_digC : p->off_flags;
    const size_t dig = p->slots * p->l * 8, top = align_up(p->slots * 4, 256);
    const size_t cbb = align_up(p->slots * cb_words((int)p->l) * 8, 256);
    p->has_c = true;
    p->off_digC = o; o += dig;
    p->off_topC = o; o += top;
    p->off_cbC = o; o += cbb;
    p->off_flags = o; o += align_up((size_t)(p->total / 256 + 8) * 4, 256);
    p->off_meta = o; o += align_up((size_t)p->slots * 4, 256);
    p->bytes = o;
    return MPFFT_OK;
}

// Signed sum of products (mpfft_sdot_*, sdot.hpp): the dot plan and its workspace, and behind it --
// whatever the sign mask -- the complement scratch (n1 limbs), D in carry-save form (n2 limbs, n2
// overflow bytes), and k_sdfix's flags, ticket counter and block-edge overflows.  A dot workspace
// laid at the front is valid as it stands.
struct SdLayout {
    size_t off_scr, off_d, off_dc, off_st, off_edge, bytes;
    long nb;   // k_sdfix's chain blocks
};
static const long SD_FIX_BLOCK = 4096;   // limbs per k_sdfix block (SDFIX_CB, MPFFT_SDOT_FIX_BLOCK)
static SdLayout sd_layout(const Plan &P)
{
    SdLayout L;
    L.nb = (P.total + SD_FIX_BLOCK - 1) / SD_FIX_BLOCK;
    size_t o = align_up(P.bytes, 256);
    L.off_scr = o; o += align_up((size_t)P.n1 * 8, 256);
    L.off_d = o; o += align_up((size_t)P.n2 * 8, 256);
    L.off_dc = o; o += align_up((size_t)P.n2, 256);
    L.off_st = o; o += align_up((size_t)(L.nb + 1) * 4, 256);
    L.off_edge = o; o += align_up((size_t)L.nb * 4, 256);
    L.bytes = o;
    return L;
}

// Squaring plan: the multiply's plan for n by n limbs -- the same split, trunc, fold, ltw and
// fuse_rows -- with operand B's arrays taken out of the layout.
static int make_plan_sqr(Plan *p, long n, unsigned long depth, unsigned long w)
{
    const int rc = make_plan(p, n, n, depth, w);
    if (rc) return rc;
    plan_drop_b(p);
    return MPFFT_OK;
}

// Multiplication by a precomputed operand.  The cache of operand B for the multiply's plan P:
// on nested plans one record per live slot, B after its inner forward transform
// (pw_pre_record_bytes); on the other families the live slots of B's fully transformed row arrays
// as those kernels read them, canonical: the limbs, then the carry limbs.
static size_t plan_pre_dig_bytes(const Plan &P) { return (size_t)P.trunc * P.l * 8; }
static size_t plan_pre_bytes(const Plan &P)
{
    if (pw_family(P) == PWF_NESTED) {
        const int lk = pwss_lk_of(P.l);
        return (size_t)P.trunc * pw_pre_record_bytes(pw_inner_limbs(P.l, lk), 1 << lk);
    }
    return plan_pre_dig_bytes(P) + align_up((size_t)P.trunc * 4, 256);
}

// The plan of a multiply against the cache: the multiply's plan for (n1, n2, depth, w) with
// operand B's arrays taken out of the layout (operand 0 alone runs the forward stages).
static int make_plan_pre(Plan *p, long n1, long n2, unsigned long depth, unsigned long w)
{
    const int rc = make_plan(p, n1, n2, depth, w);
    if (rc) return rc;
    plan_drop_b(p, false);
    return MPFFT_OK;
}

// Small matrix product (mpfft_matmul_*): R = X Y, X m x k, Y k x p, on the dot plan at K = k.  The dot
// workspace at the front -- A's and B's arrays are the staging arrays of an X and a Y operand's
// forward transform, C holds one result entry's pointwise sum -- and behind it one cache region per
// matrix entry (plan_pre_bytes, the layout mpfft_precomp_* writes), X's entries row-major, then Y's,
// at a uniform 256-byte aligned stride.  A dot workspace laid at the front is valid as it stands.
static const int MM_MAX = 4;
struct MmLayout {
    size_t off_cache, stride, bytes;
    int ncache;
};
static MmLayout mm_layout(const Plan &P, long m, long k, long p)
{
    MmLayout L;
    L.ncache = (int)(m * k + k * p);
    L.stride = align_up(plan_pre_bytes(P), 256);
    L.off_cache = align_up(P.bytes, 256);
    L.bytes = L.off_cache + (size_t)L.ncache * L.stride;
    return L;
}
// the dot plan at K = k; MPFFT_EINVAL for m, k or p outside [1, MM_MAX]
static int make_plan_matmul(Plan *p, long m, long k, long pp, long n1, long n2, unsigned long depth, unsigned long w)
{
    if (m < 1 || m > MM_MAX || k < 1 || k > MM_MAX || pp < 1 || pp > MM_MAX) {
        memset(p, 0, sizeof(*p));
        return MPFFT_EINVAL;
    }
    return make_plan_dot(p, k, n1, n2, depth, w);
}

// Negacyclic plan (nega.hpp): a b mod 2^B + 1, B = 64 L, as the length-2n negacyclic convolution
// of bits1 = B / 2n bit pieces.  The multiply's kernel families and its split for an
// untruncated transform of these (depth, w) (make_plan's choice at Tr = NR); nothing is
// truncated (a weighted transform cannot be), no fold, no fused scaling: the un-weight is the
// scaling pass.  The signed coefficients need 2 bits1 + depth + 2 <= N.
static u64 nega_scratch_limbs(const Plan &P) { return ((u64)(2 * P.n - 1) * P.bits1 + P.N + 1 + 63) / 64; }
static const int NEGA_V = 4;   // k_nwrap: limbs per thread, 256 threads
static long nega_blocks(long L) { return (L + 256 * NEGA_V - 1) / (256 * NEGA_V); }

// crt: the low-word CRT family (mpfft_mulmodw_*, negaw.hpp): a convolution of the pieces' low 32-bit
// words mod 2^32 recovers floor(c_k / p) as a signed 32-bit word, so the coefficients need only
// 2 bits1 + depth + 2 <= N + 32 -- bits1 = N / 2 for a power-of-two B; bits1 >= 32 keeps those
// words apart (below that the plain family serves the shape).
static int make_plan_mod(Plan *p, long L, unsigned long depth, unsigned long w, bool sqr, bool crt = false)
{
    memset(p, 0, sizeof(*p));
    if (L < 1 || depth < 2 || depth > 30 || w < 1 || w > 4096) return MPFFT_EINVAL;
    const u64 n2 = (u64)2 << depth, N = ((u64)1 << depth) * w, B = 64 * (u64)L;
    if (N % 64 || B % n2) return MPFFT_EINVAL;
    if (N / 64 > 4096) return MPFFT_EUNSUPPORTED;
    const u64 b = B / n2;
    if (crt && b < 32) return MPFFT_EINVAL;
    if (2 * b + depth + 2 > N + (crt ? 32 : 0)) return MPFFT_ETOOBIG;
    int rc = make_plan_split(p, 1, 1, depth, w, false, -1);
    if (rc) return rc;
    if (p->rpass && (p->l == 2048 || p->l == 4096)) {   // make_plan's split where nothing is truncated
        Plan q;
        if (make_plan_split(&q, 1, 1, depth, w, false, (int)depth / 2 + 1, p->l == 2048) == MPFFT_OK && q.rpass) *p = q;
    }
    p->nega = true;
    p->n1 = p->n2 = L;
    p->bits1 = b;
    p->j1 = p->j2 = p->len = p->trunc = 2 * p->n;
    p->Tr = p->NR;
    p->fold = 0;
    p->ltw = false;
    p->fuse_scale = false;
    p->total = (long)nega_scratch_limbs(*p);
    if (sqr) plan_drop_b(p);
    size_t o = p->off_flags;
    o += align_up((size_t)(p->total / 256 + 8) * 4, 256);
    p->off_nflags = o; o += align_up((size_t)(nega_blocks(L) + 2) * 4, 256);
    p->off_meta = o; o += align_up((size_t)p->slots * 4, 256);
    p->off_nscr = o; o += align_up((size_t)p->total * 8, 256);
    if (crt) {
        p->lowcrt = true;
        p->off_lowd = o; o += align_up((size_t)p->len * 4, 256);
    }
    p->bytes = o;
    return MPFFT_OK;
}

// Cyclic plan (cyc.hpp): a b mod 2^B - 1, B = 64 L, as the length-2n cyclic convolution of
// bits1 = B / 2n bit pieces -- what the untruncated transform computes as it stands: no weight, the
// first column pass splits the operands, the multiply's scaling at Tr = NR (fused on the wave
// plans).  Kernel families and split as make_plan_mod's.  The coefficients are non-negative,
// c_k <= 2n (2^bits1 - 1)^2, so 2 bits1 + depth + 1 <= N keeps them below 2^N.
// kind: the multiply, the square (no B arrays) or the multiply against a cached operand (Plan::pre).
enum { CYC_MUL = 0, CYC_SQR = 1, CYC_PRE = 2 };
// the scratch sum of 2n canonical coefficients below 2^N, bits1 apart: below 2^((2n - 1) bits1 + N + 1)
static u64 cyc_scratch_limbs(const Plan &P) { return ((u64)(2 * P.n - 1) * P.bits1 + P.N + 1 + 63) / 64; }
static const int CYC_V = 8;   // k_cwrap: limbs per thread, 256 threads (the ticket atomics bound it: 4 -> 8 halves them)
static long cyc_blocks(long L) { return (L + 256 * CYC_V - 1) / (256 * CYC_V); }
static const int CYC_XW = 2;  // words behind k_cwrap's flags that start as 0: the ticket counter and the overflow O
// k_cwrap's region: a look-back flag per block, the CYC_XW words, and a word per block ("a limb above limb 0
// is not all-ones": written by every block, never cleared)
static long cyc_flag_region_words(long L) { return 2 * cyc_blocks(L) + CYC_XW; }

static int make_plan_cyc(Plan *p, long L, unsigned long depth, unsigned long w, int kind)
{
    memset(p, 0, sizeof(*p));
    if (L < 1 || depth < 2 || depth > 30 || w < 1 || w > 4096) return MPFFT_EINVAL;
    if (kind != CYC_MUL && kind != CYC_SQR && kind != CYC_PRE) return MPFFT_EINVAL;
    const u64 n2 = (u64)2 << depth, N = ((u64)1 << depth) * w, B = 64 * (u64)L;
    if (N % 64 || B % n2) return MPFFT_EINVAL;
    if (N / 64 > 4096) return MPFFT_EUNSUPPORTED;
    const u64 b = B / n2;
    if (2 * b + depth + 1 > N) return MPFFT_ETOOBIG;
    int rc = make_plan_split(p, 1, 1, depth, w, false, -1);
    if (rc) return rc;
    if (p->rpass && (p->l == 2048 || p->l == 4096)) {   // make_plan's split where nothing is truncated
        Plan q;
        if (make_plan_split(&q, 1, 1, depth, w, false, (int)depth / 2 + 1, p->l == 2048) == MPFFT_OK && q.rpass) *p = q;
    }
    p->cyc = true;
    p->n1 = p->n2 = L;
    p->bits1 = b;
    p->j1 = p->j2 = p->len = p->trunc = 2 * p->n;
    p->Tr = p->NR;
    p->fold = 0;
    p->ltw = false;
    p->fuse_scale = p->wave;   // as make_plan_split's at Tr = NR
    p->total = (long)cyc_scratch_limbs(*p);
    if (kind != CYC_MUL) plan_drop_b(p, kind == CYC_SQR);
    size_t o = p->off_flags;
    o += align_up((size_t)(p->total / 256 + 8) * 4, 256);
    p->off_nflags = o; o += align_up((size_t)cyc_flag_region_words(L) * 4, 256);
    p->off_meta = o; o += align_up((size_t)p->slots * 4, 256);
    p->off_nscr = o; o += align_up((size_t)p->total * 8, 256);
    p->bytes = o;
    return MPFFT_OK;
}

// ---- (depth, w) chooser -------------------------------------------
// The reference leaves (depth, w) to its caller (mul_fft.c:3190-3191); an MPIR-style
// mpn_mul drop-in needs them picked from the operand sizes.  Candidates: every depth in
// [2, 24] and power-of-two w with a whole number of limbs per coefficient, l <= 4096, and
// room for the product (make_plan).  Predicted device time = launches x a launch cost +
// live slots (T) x the measured per-slot cost of a multiply at that coefficient size
// (CHOOSE_SLOT_NS[log2 l], from scripts/chooser_sweep.py on MI355X:
// profiles/r02/chooser_sweep.json); the cheapest candidate wins.  The round-5 re-sweep
// (profiles/r05/chooser_sweep.json: l = 2048 196 ns, l = 4096 512 ns per slot, measured at
// T = 32768 / 16384 slots) is not taken over: a linear per-slot model with those costs picks
// l = 2048 for 10^6-limb products, whose 2048 live slots fill a quarter of the GPU's
// pointwise workgroup slots -- the measured per-slot cost does not hold there.  With the r02
// table the chosen candidate is the fastest of every one timed at all four test sizes
// (profiles/r05/chooser_check.log, tests/test_gpu_chooser.py at 1.2x).  Model: a fixed cost
// (launches: ~0.045 ms for the small configurations of the sweep) + T x the marginal
// per-slot cost at that coefficient size, (ms - 0.045) / T of the sweep.
static const double CHOOSE_SLOT_NS[13] = {69.7, 26.6, 12.3, 10.4, 7.3, 6.6, 11.0, 13.2, 28.4, 98.2, 167.9, 270.0, 810.7};
static const double CHOOSE_FIXED_MS = 0.045;

// The low-word CRT family's extra term (Plan::lowcrt): k_nlowconv's 4 n^2 32-bit multiply-adds at
// CHOOSE_LOWCONV_MAC_NS each, without which the small-w candidates (many short coefficients) would
// look cheaper than they are.  Measured on MI355X by scripts/time_mulmodw.py
// (profiles/r16/mulmodw_ab.json): the stage alone takes 0.044 / 0.106 / 0.330 ms at 2n = 16384 /
// 32768 / 65536; the marginal cost between the two larger sizes is 6.96e-5 ns per multiply-add
// (the smaller sizes carry the launch and the clearing of d, which CHOOSE_FIXED_MS stands for).
static const double CHOOSE_LOWCONV_MAC_NS = 7.0e-5;

static double choose_cost(const Plan &P)
{
    const int k = ilog2(P.l);
    const double conv = P.lowcrt ? (double)P.len * (double)P.len * CHOOSE_LOWCONV_MAC_NS * 1e-6 : 0.0;
    return CHOOSE_FIXED_MS + (double)P.trunc * CHOOSE_SLOT_NS[k < 12 ? k : 12] * 1e-6 + conv;
}
