// exec.hpp -- the launches of one product on one stream: kernel dispatch, the views of a
// rank's data (View) and the stages (Exec).  Included by mpfft.hip only, after plan.hpp.
#pragma once

// ---------------------------------------------------------------------------
// kernel dispatch
// ---------------------------------------------------------------------------
typedef void (*pass_fn)(PassArgs);

template <int U>
static pass_fn pick_pass(int logg, int dir)
{
    constexpr int ML = U == 1 ? 4 : U == 2 ? 2 : 1;
    if (dir == 0) {
        switch (logg) {
        case 1: return k_pass<U, 1, 0>;
        case 2: if (ML >= 2) return k_pass<U, (ML >= 2 ? 2 : 1), 0>; break;
        case 3: if (ML >= 3) return k_pass<U, (ML >= 3 ? 3 : 1), 0>; break;
        case 4: if (ML >= 4) return k_pass<U, (ML >= 4 ? 4 : 1), 0>; break;
        }
    } else {
        switch (logg) {
        case 1: return k_pass<U, 1, 1>;
        case 2: if (ML >= 2) return k_pass<U, (ML >= 2 ? 2 : 1), 1>; break;
        case 3: if (ML >= 3) return k_pass<U, (ML >= 3 ? 3 : 1), 1>; break;
        case 4: if (ML >= 4) return k_pass<U, (ML >= 4 ? 4 : 1), 1>; break;
        }
    }
    return nullptr;
}

static size_t wpass_lds(int U, int G, int l) { return (size_t)WPB * wv_stage_slots(G, U) * 16 * (size_t)l; }

static pass_fn get_pass(int U, int logg, int dir)
{
    switch (U) {
    case 1: return pick_pass<1>(logg, dir);
    case 2: return pick_pass<2>(logg, dir);
    case 4: return pick_pass<4>(logg, dir);
    }
    return nullptr;
}

// dynamic LDS above 64 KiB must be opted into per kernel (gfx950 has 160 KiB per CU)
static void allow_lds(const void *f, size_t bytes)
{
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { last_hip_error = e_; return MPFFT_EHIP; } } while (0)
static thread_local hipError_t last_hip_error = hipSuccess;

// Where one rank's data lives.  The column layout (slot = pos * ccount + c - c0)
// feeds the column passes; the row layout (rows r0 .. r0 + rcount of `nblk` column
// blocks of ccb columns: slot = (c / ccb) * rcount * ccb + (p - r0) * ccb + c % ccb)
// feeds the row passes and the pointwise products.  On one GPU both are the same
// natural slot-major array (c0 = r0 = 0, ccount = ccb = NC, rcount = T/NC).
struct View {
    u64 *dig[2];
    u64 *cb[2];
    int *top[2];

    // the arrays it has start `slots` slots (coefficients of l limbs) further on
    void advance(long slots, long l)
    {
        for (int k = 0; k < 2; ++k)
            if (dig[k]) {
                dig[k] += slots * l;
                cb[k] += slots * cb_words((int)l);
                top[k] += slots;
            }
    }
};

struct Exec {
    const Plan &P;
    hipStream_t s;
    int nw;
    View col, row;
    View cview = {};         // the C arrays (single layout, index 0), when the plan has them
    int c0, ccount, r0, rcount, ccb, cbb;
    long cbs;
    long src_chunk = 0;      // operands are column slices (mpfft_shard.src_chunk), 0 = whole operands
    u32 *zflags = nullptr;   // non-null: the first forward column pass clears the combine's look-back flags
    long zflags_n = 0;       // (u32 words), so combine_single needs no separate fill launch
    int in_rows = 0;         // non-zero: inputs live in column rows [0, in_rows) (default: the trunc rows)
    // multiplication by a precomputed operand: the cache of operand B (plan_pre_bytes).  On a
    // Plan::pre plan the pointwise reads it (use_pre); pre_make: operand B's forward stages run
    // alone on the multiply's plan and precomp_store() writes it
    unsigned char *pre = nullptr;
    bool pre_make = false;
    bool defer_double = false;   // itft's top-level doubling is left to scale() (rows [dbl_lo, dbl_hi): 2^-depth)
    bool fold = false;           // f4 (P.fold): 2^-(depth+1) in the last inverse row pass, no scale(), combine_fold()
    bool fuse_row_last = false;  // the row DIF's last level runs inside the pointwise (k_pwss PAIR)
    // forward columns: only output rows [own_lo, own_hi) are wanted (own_hi > 0).  After the
    // first column pass a DIF splits into independent subtrees of positions; the later passes
    // skip the subtrees outside the rows (MPFFT_SHARD_FWD_COLUMNS_OWN: a rank of the replicated
    // forward columns keeps only its own rows of each column block)
    int own_lo = 0, own_hi = 0;
    // forward k_rpass passes hand their pending exponents on to the next pass of the same
    // transform (fwd_columns / fwd_rows).  Every stage still ends exact -- a transform's last
    // level leaves no pending exponent (its pass skips the closing round) -- so the stage API
    // and the sharded path run the same passes.
    bool carry_pend = !diag_env("MPFFT_NO_CARRY");
    // which hand-overs: 1 column -> column, 4 row -> row.  The receiving pass applies the
    // owed exponents (whole limb pairs) by a rotated load -- addresses and a negation, no LDS
    // round -- so its first level stays in registers and the skipped closing round is saved
    // outright.  (Round 3, when the first level took the exponents through LDS instead, the
    // hand-over paid only row -> row and column -> column at l = 4096: profiles/r03/carry_ab.txt.)
    int carry_mask() const
    {
        static const int m = [] { const char *e = diag_env("MPFFT_CARRY_MASK"); return e ? atoi(e) : -1; }();
        return m >= 0 ? m : 5;
    }
    // itft's FILL, see ifft_block.  hmin: the smallest distance of the half-adds itft1_r runs next on the
    // filled rows (0: none); habs: the pass took those of distance >= habs along (PassArgs::fill_hmin)
    struct Fill { long lo = 0, off = 0; u64 rho = 0; bool done = false; long hmin = 0, habs = 0; } fill;
    // single-GPU drivers: the half-adds after a FILL are offered to the pass that does the FILL
    bool tail_fold = false;
    // non-null: a dry run -- pass() and the pair steps append their launch to *rec and launch nothing
    // (mpfft_inv_columns_schedule)
    std::string *rec = nullptr;
    long dbl_lo = 0, dbl_hi = 0;

    Exec(const Plan &p, hipStream_t st) : P(p), s(st) { nw = P.tpb / 64; }

    // levels in the next pass when `rem` remain: the fewest passes of <= maxlogg
    // levels, balanced (C1 column inverse: 4 + 3 beats 5 + 2 by ~5 us)
    int split(int rem, bool col = false, bool inv = false) const
    {
        const int ml = inv && P.maxlogg_i ? P.maxlogg_i : col && P.maxlogg_c ? P.maxlogg_c : P.maxlogg;
        const int np = (rem + ml - 1) / ml;
        return (rem + np - 1) / np;
    }

    // k_combine1 block size: 256 comb_v() limbs (MPFFT_CB_V = 1, 2, 4, 8)
    static int comb_v()
    {
        // C3 sweep (profiles/r02/combine_cbv.txt): V = 1: 1.84 ms, 2: 0.94, 4: 0.51, 8: 0.42, 16: see there
        static const int v = [] { const char *e = diag_env("MPFFT_CB_V"); const int x = e ? atoi(e) : 8;
                                  return x == 1 || x == 2 || x == 4 || x == 16 ? x : 8; }();
        return v;
    }
    // k_combine1's form for plan P: consecutive limbs per thread (combine.hpp) where a wave's 512
    // limbs meet at most 4 coefficients, else the per-limb form (MPFFT_COMB_CT = 0: per-limb, A/B)
    static int comb_kw(const Plan &P) { return (int)((P.N + 32767) / P.bits1 + 1); }
    static bool comb_ct(const Plan &P)
    {
        static const bool no_ct = [] { const char *e = diag_env("MPFFT_COMB_CT"); return e && !strcmp(e, "0"); }();
        return comb_v() == 8 && !no_ct && comb_kw(P) <= 4;
    }
    // threads per k_combine1 block: 512 for the consecutive form (C3 combine 0.285 -> 0.266 ms
    // against 256, profiles/r05/combine_ct_ab.txt; MPFFT_COMB_NT = 256 for A/B), 256 per-limb
    static int comb_nt(const Plan &P)
    {
        static const int nt = [] { const char *e = diag_env("MPFFT_COMB_NT"); return e && atoi(e) == 256 ? 256 : 512; }();
        return comb_ct(P) ? nt : 256;
    }
    static long comb_blocks(const Plan &P, long mcount)
    {
        const long bl = (long)comb_nt(P) * comb_v();
        return (mcount + bl - 1) / bl;
    }
    u32 *comb_flags(unsigned char *ws) const { return (u32 *)(ws + P.off_flags); }
    static long comb_flag_words(const Plan &P, long mcount) { return (comb_blocks(P, mcount) + 4) / 4 * 4; }

    // what run_all sets for the whole single-GPU multiply (and the dry run of it)
    void drive_single()
    {
        defer_double = true;   // itft + scale back to back
        tail_fold = true;
        fold = P.fold != 0;    // f4: no scaling pass, the combine reads the reduced form
    }

    // single-GPU workspace: both layouts are the natural one (ws null: a dry run, no views)
    void single(unsigned char *ws)
    {
        c0 = 0;
        ccount = (int)P.NC;
        r0 = 0;
        rcount = (int)P.Tr;
        ccb = (int)P.NC;
        cbb = P.lbC;
        cbs = (long)P.Tr * P.NC;
        if (!ws) {
            col = row = cview = View{};
            return;
        }
        col.dig[0] = (u64 *)(ws + P.off_digA);
        col.top[0] = (int *)(ws + P.off_topA);
        col.cb[0] = (u64 *)(ws + P.off_cbA);
        col.dig[1] = (u64 *)(ws + P.off_digB);
        col.top[1] = (int *)(ws + P.off_topB);
        col.cb[1] = (u64 *)(ws + P.off_cbB);
        if (P.sqr) {   // no B arrays: operand 1 is operand 0 (the passes run operand 0 only)
            col.dig[1] = col.dig[0];
            col.top[1] = col.top[0];
            col.cb[1] = col.cb[0];
        }
        if (P.pre) {   // no B arrays: operand 1 is read from the cache by the pointwise alone (use_pre)
            col.dig[1] = nullptr;
            col.top[1] = nullptr;
            col.cb[1] = nullptr;
        }
        row = col;
        if (P.has_c) {
            cview.dig[0] = (u64 *)(ws + P.off_digC);
            cview.top[0] = (int *)(ws + P.off_topC);
            cview.cb[0] = (u64 *)(ws + P.off_cbC);
        }
    }

    // a Plan::pre plan's operand B: on the families that read B's row arrays, the cache holds their
    // live slots (limbs, then carry limbs; canonical, no carry masks); k_pwsp takes the records
    void use_pre(const void *d_pre)
    {
        pre = (unsigned char *)d_pre;
        if (P.pre && pre && !pwss_active()) {
            row.dig[1] = (u64 *)pre;
            row.top[1] = (int *)(pre + plan_pre_dig_bytes(P));
        }
    }

    // both layouts start `slots` slots further on (the sqrt2 plan's second half)
    void shift(long slots)
    {
        col.advance(slots, P.l);
        row = col;
        cview.advance(slots, P.l);
    }

  private:
    // every launch of Exec: the LDS opt-in (nothing at or below 64 KiB), the launch on s, its error
    template <typename F, typename... A>
    int launch(F f, dim3 grid, dim3 block, size_t lds, A... args)
    {
        allow_lds((const void *)f, lds);
        hipLaunchKernelGGL(f, grid, block, lds, s, args...);
        HIPCHK(hipGetLastError());
        return MPFFT_OK;
    }

  public:
    // rotation staging buffers for a G-coefficient pass: as many as fit in 64 KiB
    int stage_bufs(int G) const
    {
        long fit = (64L * 1024) / (16L * P.l);
        if (fit < 1) fit = 1;
        return (int)(fit < G ? fit : G);
    }

    // k_rpass takes a pass unless it needs a canonical store, has zero inputs outside the
    // split, or some level rotation is not a whole number of limb pairs
    int rpass_mode(const PassArgs &a, int logg, int dir) const
    {
        if (!P.rpass || logg > (dir ? rp_maxlogg_dit((int)P.l) : rp_maxlogg_fwd4((int)P.l)) || a.canon || a.rho % 128) return -1;
        if (dir == 0) {
            if (a.scale_e || a.tw_mode == 2) return -1;
            if (a.src[0] || a.src[1]) return a.tw_mode || a.pcarry ? -1 : 2;
            if (a.zero_from < (1 << a.lbM)) return -1;
            if (a.tw_mode == 1) return a.pcarry ? -1 : 1;
            return a.pcarry ? 3 : 0;
        }
        if (a.tw_mode == 1) return -1;
        const bool ltw = a.tw_mode == 3, hl = a.lvl0 + logg == a.lbM;   // 3: the inverse twiddle on load (it takes scale_e too)
        if (ltw && !hl) return -1;
        const int gx = !ltw && (a.tw_mode == 2 || a.scale_e) ? 1 : 0;
        if (a.fill_off && gx) return -1;
        return gx | (hl ? 2 : 0) | (a.fill_off ? 4 : 0) | (ltw ? 8 : 0);
    }

    // the k_rpass mode pass() launches for these arguments, -1: another kernel family
    int rp_mode(const PassArgs &a, int logg, int dir) const
    {
        int rm = rpass_mode(a, logg, dir);
        static const int rmask = [] { const char *e = diag_env("MPFFT_RPASS_OFF"); return e ? atoi(e) : 0; }();
        if (rm >= 0 && (rmask >> (4 * dir + rm) & 1)) rm = -1;   // diagnostics: bit 4 dir + mode off
        return rm;
    }

    // levels of a pass whose arguments mk(k) builds: k, unless k_rpass declines that pass and
    // k_bpass cannot hold 2^k coefficients in LDS (k_rpass takes more levels per pass than
    // k_bpass fits: three at l = 4096, four inverse at l = 2048) -- then k_bpass's limit
    template <typename MK>
    int fit(int k, int dir, MK mk) const
    {
        if (!P.big || !P.bp_lg || k <= P.bp_lg || rp_mode(mk(k), k, dir) >= 0) return k;
        return P.bp_lg;
    }

    // the groups a pass launches: all 2^(lbM - logg) per sub-array, except in a forward pass, where
    // only blocks of 2^(lbM - lvl0) positions meeting [need_lo, need) are live -- the kernels return
    // at once for the others, but a launched-and-returning 1024-thread workgroup with 147 KB of LDS
    // still cost C3's second column pass 0.3 ms (931 -> 636 us, profiles/r06/live_groups_ab.txt):
    // the grid covers [grp0, grp0 + ngroups) only
    static void live_groups(PassArgs &a, int logg, int dir)
    {
        a.ngroups = 1 << (a.lbM - logg);
        a.grp0 = 0;
        if (dir != 0) return;
        const int slg = a.lbM - a.lvl0, lobits = slg - logg;
        const long nh = 1L << a.lvl0;
        const long hlo = std::min<long>(nh, a.need_lo > 0 ? (long)a.need_lo >> slg : 0);
        const long hhi = std::min<long>(nh, ((long)a.need + (1L << slg) - 1) >> slg);
        if (hhi > hlo) {
            a.grp0 = (int)(hlo << lobits);
            a.ngroups = (int)((hhi - hlo) << lobits);
        }
    }

    int pass(PassArgs a, int logg, int dir, int nops)
    {
        const int rm = rp_mode(a, logg, dir);
        if (rec) {
            char ln[160];
            int n = rm >= 0 ? snprintf(ln, sizeof ln, "k_rpass<%d,%d,%d,%d> pos %d+%d", logg, (int)P.l / 1024, dir, rm, a.pos_off, 1 << a.lbM)
                            : snprintf(ln, sizeof ln, "pass<%d,%d> pos %d+%d", logg, dir, a.pos_off, 1 << a.lbM);
            if (rm >= 0 && !rp_get((int)P.l, logg, dir, rm)) return MPFFT_EUNSUPPORTED;   // as the launch below
            if (a.fill_off) n += snprintf(ln + n, sizeof ln - n, " fill lo=%d off=%d", a.fill_lo, a.fill_off);
            if (a.fill_hmin) n += snprintf(ln + n, sizeof ln - n, " halfadd %d..%d", a.fill_off / 2, a.fill_hmin);
            *rec += ln;
            *rec += '\n';
            return MPFFT_OK;
        }
        // each family: its kernel, LDS bytes, threads per block and groups per block
        pass_fn f = nullptr;
        size_t lds = 0;
        unsigned nt = 0;
        int gpb = 1;
        bool stamps = false;
        if (rm >= 0) {
            f = rp_get((int)P.l, logg, dir, rm);
            static const size_t pad = [] { const char *e = diag_env("MPFFT_RPASS_LDSPAD"); return e ? (size_t)atol(e) : 0; }();
            static const int abl = [] { const char *e = diag_env("MPFFT_ABLATE"); return e ? atoi(e) : 0; }();
            a.ablate = abl;
            lds = rp_lds((int)P.l, logg) + pad;   // pad: diagnostics (one workgroup per CU)
            nt = (unsigned)rp_nt((int)P.l, logg, dir);
            static const bool rp_stamps = diag_env("MPFFT_RP_STAMPS") != nullptr;
            stamps = rp_stamps;
        } else if (P.big) {
            // limb-aligned kernel unless some rotation of the pass has a sub-limb part
            const bool gen = (a.rho % 64) || (a.tw_mode && a.tw_w % 64) || (a.scale_e % 64);
            f = gen ? bp_get_gen(logg, dir) : bp_get(logg, dir);
            lds = bp_lds_need((int)P.l, 1 << logg);
            nt = (unsigned)(64 * bp_waves((int)P.l, logg));
            static const bool bp_stamps = diag_env("MPFFT_BP_STAMPS") != nullptr;
            stamps = bp_stamps;
        } else if (P.wave && P.lds) {
            f = wv_fns(P.wU, P.wfull).lpass(logg, dir);
            lds = ((size_t)16 * P.l) << logg;
            nt = 32u << logg;
        } else if (P.wave) {   // a wave per group, WPB of them in a block
            const char *e = diag_env("MPFFT_ABLATE");
            a.ablate = e ? atoi(e) : 0;
            f = wv_fns(P.wU, P.wfull).pass(logg, dir);
            lds = wpass_lds(P.wU, 1 << logg, (int)P.l);
            nt = 64 * WPB;
            gpb = WPB;
        } else {
            f = get_pass(P.U, logg, dir);
            a.nbuf = stage_bufs(1 << logg);
            lds = lds_bytes((int)P.l, a.nbuf, 1 << logg, P.U, nw);
            nt = (unsigned)P.tpb;
        }
        if (!f) return MPFFT_EUNSUPPORTED;
        live_groups(a, logg, dir);
        const long groups = (long)a.nsub * a.ngroups;
        const dim3 grid((unsigned)((groups + gpb - 1) / gpb), (unsigned)nops);
        if (stamps) return bp_stamped(f, grid, nt, lds, a, logg, dir);
        return launch(f, grid, dim3(nt), lds, a);
    }

    // diagnostics only: per-workgroup phase stamps (8 ticks each, written by the kernel through
    // its debug pointer) of one launch over n workgroups
    struct Stamps {
        size_t n = 0;
        unsigned long long *d = nullptr;
        long cnt = 0;                       // workgroups that ran to their last stamp
        unsigned long long t0 = ~0ull, t1 = 0;   // their first and last tick
        double avg[8] = {0};                // avg[k]: ticks from the stamp taken before to stamp k
    };
    int stamps_begin(Stamps &st, size_t n)
    {
        st.n = n;
        HIPCHK(hipMalloc((void **)&st.d, n * 64));
        HIPCHK(hipMemsetAsync(st.d, 0, n * 64, s));
        return MPFFT_OK;
    }
    // copy back, average over the workgroups that ran, free
    int stamps_end(Stamps &st)
    {
        std::vector<unsigned long long> h(st.n * 8);
        HIPCHK(hipMemcpyAsync(h.data(), st.d, st.n * 64, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t w = 0; w < st.n; ++w) {
            const unsigned long long *q = h.data() + 8 * w;
            if (!q[7]) continue;   // skipped group (past the truncation point)
            ++st.cnt;
            if (q[0] < st.t0) st.t0 = q[0];
            if (q[7] > st.t1) st.t1 = q[7];
            unsigned long long prev = q[0];
            for (int k = 1; k < 8; ++k)
                if (q[k]) { st.avg[k] += (double)(q[k] - prev); prev = q[k]; }
        }
        for (int k = 1; k < 8; ++k) st.avg[k] /= st.cnt;
        (void)hipFree(st.d);
        return MPFFT_OK;
    }

    // diagnostics only (MPFFT_BP_STAMPS, MPFFT_RP_STAMPS): run one pass launch with phase stamps
    // and print the average phase lengths (s_memtime ticks) of the working groups
    int bp_stamped(pass_fn f, dim3 grid, unsigned nthr, size_t lds, PassArgs a, int logg, int dir)
    {
        Stamps st;
        int rc;
        if ((rc = stamps_begin(st, (size_t)grid.x * grid.y))) return rc;
        a.dbg = st.d;
        if ((rc = launch(f, grid, dim3(nthr), lds, a)) || (rc = stamps_end(st))) return rc;
        const double *v = st.avg;
        fprintf(stderr, "%s logg=%d dir=%d l=%ld groups=%ld/%zu span=%llu ticks: load %.0f lv0 %.0f lv1 %.0f lv2 %.0f fin %.0f canon/hx %.0f store %.0f\n", nthr == RP_NT || nthr == 1024 ? "rp_stamps" : "bp_stamps",
                logg, dir, P.l, st.cnt, st.n, st.t1 - st.t0, v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        return MPFFT_OK;
    }

    PassArgs base_args(const View &v) const
    {
        PassArgs a;
        memset(&a, 0, sizeof(a));
        for (int k = 0; k < 2; ++k) {
            a.dig[k] = v.dig[k];
            a.cb[k] = v.cb[k];
            a.top[k] = v.top[k];
        }
        a.bits1 = P.bits1;
        a.N = P.N;
        a.l = (int)P.l;
        a.pbb = 30;
        a.jNC = P.NC;
        return a;
    }

    // column layout passes over this rank's ccount columns
    PassArgs col_args() const
    {
        PassArgs a = base_args(col);
        a.sub_stride = 1;
        a.pos_stride = ccount;
        a.nsub = ccount;
        a.sub_off = c0;
        return a;
    }

    // row layout passes over this rank's rcount rows
    PassArgs row_args() const
    {
        PassArgs a = base_args(row);
        a.lbM = P.lbC;
        a.rho = (u64)P.w * P.NR;
        a.sub_stride = ccb;
        a.pos_stride = 1;
        a.pbb = cbb;
        a.pbs = cbs;
        a.nsub = rcount;
        a.sub_off = r0;
        a.zero_from = (int)P.NC;
        a.need = (int)P.NC;
        a.tw_w = (u64)P.w;
        a.tw_lbR = P.lbR;
        return a;
    }

    // stage 1: split + forward truncated column DIF (length NR, root 2^(w NC))
    // operand `op` alone (0 or 1) in slot 0 of the pass arguments, one grid row (nops = 1);
    // op < 0: both operands (grid rows 0, 1)
    static PassArgs only(PassArgs a, int op)
    {
        if (op == 1) {
            a.dig[0] = a.dig[1];
            a.cb[0] = a.cb[1];
            a.top[0] = a.top[1];
            a.src[0] = a.src[1];
            a.nsrc[0] = a.nsrc[1];
        }
        return a;
    }

    // Pending exponents across forward passes (carry_pend): a k_rpass DIF pass whose successor
    // in the same transform is also a k_rpass DIF pass skips its closing rotation round (the
    // last level's pending exponents, one LDS round trip of all G coefficients) and leaves them
    // in HBM; the successor folds them into its first level's partner rotations
    // (PassArgs::pcarry).  Nothing crosses a stage: the last pass of a transform owes nothing.
    PassArgs col_pass_args(int lvl) const
    {
        PassArgs a = col_args();
        a.zero_from = a.zero_op[0] = a.zero_op[1] = (int)P.NR;
        a.lbM = P.lbR;
        a.lvl0 = lvl;
        a.rho = (u64)P.w * P.NC;
        a.need = (int)P.Tr;
        if (own_hi > 0) {   // only rows [own_lo, own_hi) wanted: skip the DIF subtrees outside them
            a.need = own_hi < a.need ? own_hi : a.need;
            a.need_lo = own_lo;
        }
        return a;
    }

    // The passes of one forward (DIF) transform of L levels: mk(lvl, k) builds the arguments of a
    // k-level pass at level lvl; col: column passes (split's levels per pass); cbit: the
    // transform's carry_mask bit; operands as in only().
    template <typename MK>
    int fwd_passes(int L, bool col, int cbit, int nops, int op, MK mk)
    {
        int lvl = 0, pend0 = 0;   // the data owe the pending exponents of levels [pend0, lvl)
        while (lvl < L) {
            auto mkp = [&](int kk) {
                PassArgs b = mk(lvl, kk);
                b.pcarry = lvl - pend0;
                return b;
            };
            const int k = fit(split(L - lvl, col), 0, mkp);
            PassArgs a = mkp(k);
            if (carry_pend && (carry_mask() & cbit) && lvl + k < L && rp_mode(a, k, 0) >= 0) {
                const int k2 = split(L - lvl - k, col);
                PassArgs n = mk(lvl + k, k2);
                n.pcarry = k;   // it would owe this pass's levels
                a.pkeep = rp_mode(n, k2, 0) >= 0;
            }
            int rc = op < 0 ? pass(a, k, 0, nops) : pass(only(a, op), k, 0, 1);
            if (rc) return rc;
            // a keeping pass owes its own levels only (a receiving pass applies what it was
            // owed on load: rotated load, k_rpass MODE 3)
            pend0 = a.pkeep ? lvl : lvl + k;
            lvl += k;
        }
        return MPFFT_OK;
    }

    int fwd_columns(const u64 *srcA, long nA, const u64 *srcB, long nB, int nops, int op = -1)
    {
        return fwd_passes(P.lbR, true, 1, nops, op, [&](int lvl, int) {
            PassArgs a = col_pass_args(lvl);
            if (lvl == 0) {
                a.src[0] = srcA; a.nsrc[0] = nA;
                a.src[1] = srcB; a.nsrc[1] = nB;
                a.src_chunk = src_chunk;
                a.zero_from = in_rows ? in_rows : (int)P.Tr;
                a.zero_op[0] = a.zero_op[1] = a.zero_from;
                if (srcA && srcB && !src_chunk && !in_rows) {
                    // whole operands split by this pass: operand op ends in row ceil(j_op / NC) - 1, far
                    // below the product's truncation row (C3: 78 of 156).  k_rpass takes its own
                    // operand's bound by grid row; the other families take the larger of the two
                    a.zero_op[0] = (int)rp_zero_row(P.j1, P.NC, P.Tr);
                    a.zero_op[1] = (int)rp_zero_row(P.j2, P.NC, P.Tr);
                    if (op >= 0) a.zero_op[0] = a.zero_op[1] = a.zero_op[op];   // only(a, op): grid row 0
                    a.zero_from = std::max(a.zero_op[0], a.zero_op[1]);
                }
                a.zp = op == 1 ? nullptr : zflags;   // the combine flags are cleared by operand 0's pass
                a.zn = zflags_n;
            }
            return a;
        });
    }

    // the last row level fused into k_pwss: slot pairs (2i, 2i + 1) of a row adjacent (any row
    // layout with column blocks of ccb >= 2), a nested negacyclic pointwise with its fused-pair
    // instance, and a row pass left to apply the MFA twiddle
    // row DIF levels fused into the pointwise (0, 1 or 2)
    int row_fused() const
    {
        static const bool off = [] { const char *e = diag_env("MPFFT_FUSE_ROW"); return e && !strcmp(e, "0"); }();
        const int f = P.fuse_rows;
        // (k_pwsx writes to the cache: precomputing needs no C arrays)
        return fuse_row_last && !off && f && (cview.dig[0] || pre_make) && pw_pair_kernel(P.l, f) && ccb >= (1 << f) ? f : 0;
    }

    int row_levels() const { return P.lbC - row_fused(); }

    PassArgs row_pass_args(int lvl, int k, int L) const
    {
        PassArgs a = row_args();
        a.lvl0 = lvl;
        a.tw_mode = lvl == 0 ? 1 : 0;
        // canonical pointwise inputs, except for k_pwss (it loads the reduced form)
        if (lvl + k == L) a.canon = pwss_active() ? 0 : 1;
        return a;
    }

    // stage 2: MFA twiddle + row DIF (length NC, root 2^(w NR)), canonical out
    int fwd_rows(int nops, int op = -1)
    {
        const int L = row_levels();
        return fwd_passes(L, false, 4, nops, op, [&](int lvl, int k) { return row_pass_args(lvl, k, L); });
    }

    // the nested negacyclic pointwise carries this plan (it loads the reduced form)
    bool pwss_active() const { return pw_family(P) == PWF_NESTED; }

    long pw_count = 0;   // > 0: the pointwise covers this many slots from the row views (a row chunk of one column block)

    // the nested negacyclic pointwise (pkernels.hpp): k_pwss, k_pwsq on a squaring plan, or k_pwsp
    // against the cache on a Plan::pre plan
    int pointwise_nested(long cnt)
    {
        const int lk = pwss_lk_of(P.l), M = pw_inner_limbs(P.l, lk), fz = row_fused();
        pw_fn f = pw_get(M, lk, fz);
        pw_sq_fn fs = P.sqr ? pw_get_sqr(M, lk, fz) : nullptr;
        pw_mulpre_fn fp = P.pre ? pw_get_mulpre(M, lk, fz) : nullptr;
        if (!f || (P.sqr && !fs)) return MPFFT_EUNSUPPORTED;   // a missing squaring instance is an error
        if (P.pre && (!fp || !pre)) return MPFFT_EUNSUPPORTED;  // and so is a missing cached one
        const size_t lds = pw_lds(M, 1 << lk, (int)P.l);
        const dim3 grid((unsigned)cnt), block(1u << lk);
        static const bool stamps = diag_env("MPFFT_PW_STAMPS") != nullptr;
        Stamps st;   // diagnostics only
        int rc;
        if (stamps && (rc = stamps_begin(st, (size_t)cnt))) return rc;
        if (fp)   // against the cache: the same grid, block and LDS
            rc = launch(fp, grid, block, lds, row.dig[0], row.cb[0], row.top[0], (const unsigned char *)pre, (int)P.l,
                        cview.dig[0], cview.cb[0], cview.top[0], st.d);
        else if (fs)   // squaring plan: the same grid, block and LDS
            rc = launch(fs, grid, block, lds, row.dig[0], row.cb[0], row.top[0], (int)P.l, cview.dig[0], cview.cb[0],
                        cview.top[0], st.d);
        else
            rc = launch(f, grid, block, lds, row.dig[0], row.cb[0], row.top[0], (const u64 *)row.dig[1],
                        (const u64 *)row.cb[1], (const int *)row.top[1], (int)P.l, cview.dig[0], cview.cb[0], cview.top[0],
                        st.d);
        if (rc) return rc;
        if (fz > 0) {   // the product lives in C from here on (single layout: rows == columns)
            row.dig[0] = col.dig[0] = cview.dig[0];
            row.cb[0] = col.cb[0] = cview.cb[0];
            row.top[0] = col.top[0] = cview.top[0];
        }
        if (stamps) {
            if ((rc = stamps_end(st))) return rc;
            const double *v = st.avg;
            fprintf(stderr, "pw_stamps M=%d lk=%d slots=%ld/%ld: load %.0f fwdA %.0f fwdB %.0f mul %.0f inv %.0f final %.0f out %.0f\n",
                    M, lk, st.cnt, cnt, v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        }
        return MPFFT_OK;
    }

    // operand B's live slots in the row arrays -> the cache (pre_make): k_pwsx on nested plans (the
    // row levels the plan fuses run in its loaders), else a copy of the limbs and carry limbs
    // op: the operand whose row arrays are stored (the matrix products cache operand 0's as well)
    int precomp_store(int op = 1)
    {
        const long cnt = (long)rcount * P.NC;
        if (!pre) return MPFFT_EINVAL;
        if (!pwss_active()) {
            HIPCHK(hipMemcpyAsync(pre, row.dig[op], plan_pre_dig_bytes(P), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(pre + plan_pre_dig_bytes(P), row.top[op], (size_t)cnt * 4, hipMemcpyDeviceToDevice, s));
            return MPFFT_OK;
        }
        const int lk = pwss_lk_of(P.l), M = pw_inner_limbs(P.l, lk), fz = row_fused();
        pw_pre_fn f = pw_get_pre(M, lk, fz);
        if (!f) return MPFFT_EUNSUPPORTED;
        return launch(f, dim3((unsigned)cnt), dim3(1u << lk), pw_lds(M, 1 << lk, (int)P.l), (const u64 *)row.dig[op],
                      (const u64 *)row.cb[op], (const int *)row.top[op], (int)P.l, pre, (unsigned long long *)nullptr);
    }

    // ---- small matrix products (mm_layout): one result entry's pointwise sum -------------------
    // C <- (acc: C +) sum_{i < kk} cache ea[i] * cache eb[i] over the live slots; caches: region e at
    // caches + e stride.  Nested plans: k_pwmm on the records.  Elsewhere the caches hold transformed
    // row arrays: per term a copy of cache ea[i] into the staging array (the first term of a fresh
    // sum: into C itself), the plan's pointwise in place with B read from cache eb[i], and k_slotacc
    // for every term but that first.  The views are left as they were.
    int pointwise_mm(const unsigned char *caches, size_t stride, int kk, const int *ea, const int *eb, bool acc)
    {
        const long cnt = (long)rcount * P.NC;
        if (cnt == 0 || !cview.dig[0] || !caches || kk < 1 || kk > MM_MAX) return MPFFT_EINVAL;
        if (pwss_active()) {
            const int lk = pwss_lk_of(P.l), M = pw_inner_limbs(P.l, lk);
            const size_t lds = pw_lds(M, 1 << lk, (int)P.l);
            const dim3 grid((unsigned)cnt), block(1u << lk);
            // one launch for all kk terms: the sum in the inner ring, one inner inverse (against kk launches of
            // one term each, accumulating in C: 0.73 of their time at M = 18)
            pw_mm_fn f = pw_get_mm(M, lk, acc);
            if (!f) return MPFFT_EUNSUPPORTED;   // a missing instance is an error
            unsigned pa = 0, pb = 0;
            for (int i = 0; i < kk; ++i) {
                pa |= (unsigned)ea[i] << (8 * i);
                pb |= (unsigned)eb[i] << (8 * i);
            }
            return launch(f, grid, block, lds, caches, (unsigned long long)stride, kk, pa, pb, (int)P.l, cview.dig[0],
                          cview.cb[0], cview.top[0]);
        }
        const View row0 = row, col0 = col;
        const unsigned char *pre0 = pre;
        int rc = MPFFT_OK;
        for (int i = 0; i < kk && !rc; ++i) {
            const bool first = i == 0 && !acc;
            row = row0;
            col = col0;
            if (first) view_op0(cview);
            const unsigned char *xa = caches + (size_t)ea[i] * stride;
            pre = (unsigned char *)(caches + (size_t)eb[i] * stride);
            row.dig[1] = (u64 *)pre;
            row.top[1] = (int *)(pre + plan_pre_dig_bytes(P));
            // the cached operand is canonical: its limbs, its carry limbs, no carry masks
            HIPCHK(hipMemcpyAsync(row.dig[0], xa, plan_pre_dig_bytes(P), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(row.top[0], xa + plan_pre_dig_bytes(P), (size_t)cnt * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemsetAsync(row.cb[0], 0, (size_t)cnt * cb_words((int)P.l) * 8, s));
            rc = pointwise();
            if (!rc && !first) rc = slot_acc(cnt);
        }
        row = row0;
        col = col0;
        pre = (unsigned char *)pre0;
        return rc;
    }

    int pointwise()
    {
        const long cnt = pw_count > 0 ? pw_count : (long)rcount * P.NC;
        if (cnt == 0) return MPFFT_OK;
        if (P.pre && !pre) return MPFFT_EINVAL;
        // Squaring plans reach the four families after the nested one with A's arrays as B as well
        // (Exec::single).  That is safe in place: in each of k_pwm2, k_pwm, k_pw and k_pointwise a
        // thread reads topB[slot] and its limbs of B at the very point where it reads topA[slot]
        // and the same limbs of A (into registers or LDS), and A is only written by
        // normalize_store at the end -- B == A adds no read that the multiply does not already
        // order before that write (nothing is __restrict__).
        const dim3 grid((unsigned)cnt);
        u64 *dig = row.dig[0], *cb = row.cb[0];
        int *top = row.top[0];
        const u64 *digB = row.dig[1];
        const int *topB = row.top[1];
        const int l = (int)P.l;
        switch (pw_family(P)) {
        case PWF_NESTED: return pointwise_nested(cnt);
        case PWF_PWM2: {
            const int nw = l / 256;
            void (*f)(u64 *, u64 *, int *, const u64 *, const int *, int, int) =
                diag_env("MPFFT_PWM2_D4") && nw <= 8 ? k_pwm2<4, 2, 4> : k_pwm2<4, 2, 2>;   // D = 4: more VGPRs, slower at C2
            const char *ea = diag_env("MPFFT_PWABLATE");   // timing experiments only: 1 = no MFMA phase
            return launch(f, grid, dim3(64 * nw), pwm_lds_bytes(l, 4, nw), dig, cb, top, digB, topB, l, ea ? atoi(ea) : 0);
        }
        case PWF_PWM: {
            const int nw = std::min(l / 128, 16);
            const int U = l / (64 * nw);
            void (*f)(u64 *, u64 *, int *, const u64 *, const int *, int) = nullptr;
            if (U == 2) f = k_pwm<2, 1>;
            else if (U == 4) f = k_pwm<4, 2>;
            else return MPFFT_EUNSUPPORTED;
            return launch(f, grid, dim3(64 * nw), pwm_lds_bytes(l, U, nw), dig, cb, top, digB, topB, l);
        }
        case PWF_PW: {
            const int R = l >= 2048 ? 8 : 4;
            const int L = 2 * l;
            const int tpb = (L / R + 63) / 64 * 64;   // whole waves (threads past L/R idle in the MAC loop)
            const size_t lds = (size_t)3 * L * 4 + (norm_scr_u64(1, R / 2, 16) + 2) * 8;
            void (*f)(u64 *, u64 *, int *, const u64 *, const int *, int) = R == 8 ? k_pw<8> : k_pw<4>;
            return launch(f, grid, dim3(tpb), lds, dig, cb, top, digB, topB, l);
        }
        case PWF_POINTWISE: break;
        }
        const size_t lds = (size_t)3 * 2 * P.l * 4 + (norm_scr_u64(1, P.U, 16) + 2) * 8;
        void (*f)(u64 *, u64 *, int *, const u64 *, const int *, int, u64) = nullptr;
        switch (P.U) {
        case 1: f = k_pointwise<1>; break;
        case 2: f = k_pointwise<2>; break;
        case 4: f = k_pointwise<4>; break;
        }
        return launch(f, grid, dim3(P.tpb), lds, dig, cb, top, digB, topB, l, P.N);
    }

    // ---- sums of products (make_plan_dot): the C arrays are the accumulator ------------------
    // the row and column views' operand 0 from here on: the arrays of v's operand 0
    void view_op0(const View &v)
    {
        row.dig[0] = col.dig[0] = v.dig[0];
        row.cb[0] = col.cb[0] = v.cb[0];
        row.top[0] = col.top[0] = v.top[0];
    }

    // C[slot] <- C[slot] + A[slot] over the live slots (k_slotacc, dot.hpp)
    int slot_acc(long cnt)
    {
        void (*f)(u64 *, u64 *, int *, const u64 *, const u64 *, const int *, int) = nullptr;
        switch (P.U) {
        case 1: f = k_slotacc<1>; break;
        case 2: f = k_slotacc<2>; break;
        case 4: f = k_slotacc<4>; break;
        }
        if (!f) return MPFFT_EUNSUPPORTED;
        return launch(f, dim3((unsigned)cnt), dim3(P.tpb), lds_bytes((int)P.l, 0, 1, P.U, nw), cview.dig[0], cview.cb[0],
                      cview.top[0], (const u64 *)row.dig[0], (const u64 *)row.cb[0], (const int *)row.top[0], (int)P.l);
    }

    // one term's pointwise, the views on that term's transformed operands.
    // acc: C <- C + A B: k_pwsa on nested plans (A and B only read), else the product in place in A
    // as pointwise() forms it and k_slotacc behind it.
    // !acc (the first term): pointwise() as it stands -- the fused k_pwss writes C; the kernels that
    // work in place leave the product in the views' operand 0, which the caller has pointed at C
    // (run_dot) or copies there (the stage entry).
    int pointwise_dot(bool acc)
    {
        const long cnt = (long)rcount * P.NC;
        if (cnt == 0 || !cview.dig[0]) return MPFFT_EINVAL;
        if (!acc) return pointwise();
        if (!pwss_active()) {
            int rc = pointwise();
            return rc ? rc : slot_acc(cnt);
        }
        const int lk = pwss_lk_of(P.l), M = pw_inner_limbs(P.l, lk), fz = row_fused();
        pw_acc_fn f = pw_get_acc(M, lk, fz);
        if (!f) return MPFFT_EUNSUPPORTED;   // a missing accumulating instance is an error
        return launch(f, dim3((unsigned)cnt), dim3(1u << lk), pw_lds(M, 1 << lk, (int)P.l), (const u64 *)row.dig[0],
                      (const u64 *)row.cb[0], (const int *)row.top[0], (const u64 *)row.dig[1], (const u64 *)row.cb[1],
                      (const int *)row.top[1], (int)P.l, cview.dig[0], cview.cb[0], cview.top[0],
                      (unsigned long long *)nullptr);
    }

    // the live slots of the views' operand 0 -> C (the stage entry's first term on the in-place kernels)
    int copy_to_c()
    {
        const size_t cnt = (size_t)rcount * P.NC;
        HIPCHK(hipMemcpyAsync(cview.dig[0], row.dig[0], cnt * P.l * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(cview.cb[0], row.cb[0], cnt * cb_words((int)P.l) * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(cview.top[0], row.top[0], cnt * 4, hipMemcpyDeviceToDevice, s));
        return MPFFT_OK;
    }

    // ---- signed sums of products (sdot.hpp) on the regions behind the dot workspace (sd_layout) ----
    static SdArgs sd_args(const Plan &P, unsigned char *ws)
    {
        const SdLayout L = sd_layout(P);
        SdArgs d;
        memset(&d, 0, sizeof(d));
        d.Dl = (u64 *)(ws + L.off_d);
        d.Dc = ws + L.off_dc;
        d.st = (u32 *)(ws + L.off_st);
        d.edge = (int *)(ws + L.off_edge);
        d.n1 = P.n1;
        d.n2 = P.n2;
        d.total = P.total;
        d.nb = L.nb;
        return d;
    }
    static u64 *sd_scratch(const Plan &P, unsigned char *ws) { return (u64 *)(ws + sd_layout(P).off_scr); }

    // a negative term's pre-pass: ~a into the scratch, D <- b (init) or D <- D + b
    int sd_neg(const u64 *a, const u64 *b, unsigned char *ws, bool init)
    {
        const long n = P.n1 > P.n2 ? P.n1 : P.n2;
        return launch(k_sdneg, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, a, b, sd_scratch(P, ws), sd_args(P, ws), init ? 1 : 0);
    }

    // r <- r + D - (D << 64 n1) over P.total limbs: the block edges and the cleared flags, then the chain
    int sd_fix(u64 *r, unsigned char *ws)
    {
        const SdArgs d = sd_args(P, ws);
        if (int rc = launch(k_sdedge, dim3((unsigned)((d.nb + 256) / 256)), dim3(256), 0, d, (const u64 *)r)) return rc;
        return launch(k_sdfix, dim3((unsigned)d.nb), dim3(SDFIX_NT), 0, d, r);
    }

    // stage 4: row DIT inverse, MFA un-twiddle at the end
    int inv_rows()
    {
        int hi = P.lbC;
        while (hi > 0) {
            auto mk = [&](int kk) {
                PassArgs b = row_args();
                b.lvl0 = hi - kk;
                b.tw_mode = (hi - kk == 0 && !(fold && P.ltw)) ? 2 : 0;   // (ltw: on load in the column blocks)
                if (fold && !P.ltw && hi - kk == 0) b.scale_e = 2 * P.N - (u64)(P.depth + 1);   // the scaling rides in the un-twiddle
                return b;
            };
            const int k = fit(split(hi, false, true), 1, mk);
            PassArgs a = mk(k);
            int rc = pass(a, k, 1, 1);
            if (rc) return rc;
            hi -= k;
        }
        return MPFFT_OK;
    }

    // full inverse (DIT) over block [off, off + m) of every local column
    int ifft_block(long off, long m)
    {
        if (int rc = flush_chain()) return rc;
        const int lbM = ilog2(m);
        int hi = lbM;
        while (hi > 0) {
            auto mk = [&](int kk) {
                PassArgs b = col_args();
                b.lbM = lbM;
                b.lvl0 = hi - kk;
                b.rho = rho_blk(m);
                b.pos_off = (int)off;
                b.zero_from = (int)m;
                b.need = (int)m;
                if (P.fuse_scale && hi - kk == 0 && m == P.NR) {   // the whole column inverse is this block
                    b.scale_e = 2 * P.N - (u64)(P.depth + 1);
                    b.canon = 1;
                }
                if (fold && P.ltw && hi == lbM) {   // the block's first pass: inverse MFA twiddle + scaling on load
                    b.tw_mode = 3;
                    b.tw_w = (u64)P.w;
                    b.tw_lbR = P.lbR;
                    b.scale_e = 2 * P.N - (u64)(P.depth + 1);
                }
                return b;
            };
            const int k = fit(split(hi, true, true), 1, mk);
            PassArgs a = mk(k);
            if (hi - k == 0 && fill.off) {   // the block's last pass also does the pending FILL step
                PassArgs f = a;
                f.fill_lo = (int)fill.lo;
                f.fill_off = (int)fill.off;
                f.fill_rho = fill.rho;
                // the half-adds whose row pairs (p, p + d) sit in one group of this pass: d a multiple
                // of its position step 2^(lbM - k) (d <= fill.off / 2 = 2^(k - 1) steps always is)
                const long hm = std::max(fill.hmin, 1L << (lbM - k));
                if (fill.hmin && hm <= fill.off / 2) f.fill_hmin = (int)hm;
                const int fm = rp_mode(f, k, 1);
                if (fm >= 0 && rp_get((int)P.l, k, 1, fm)) {
                    a = f;
                    fill.done = true;
                    fill.habs = f.fill_hmin;
                }
            }
            int rc = pass(a, k, 1, 1);
            if (rc) return rc;
            hi -= k;
        }
        return MPFFT_OK;
    }

    // The truncated inverse's tail (Exec::chain): TWOXMY steps on one row range are held back
    // and run together with the IBFLY that consumes their rows (k_rchain), so those rows are
    // read once; anything else flushes them first.
    struct Chain { long off = 0, t = 0; int n = 0; long h[3] = {0, 0, 0}; } chain;

    int flush_chain()
    {
        const Chain c = chain;
        chain.n = 0;
        for (int j = 0; j < c.n; ++j) {
            int rc = pairop_now(OP_TWOXMY, c.off, c.h[j], 0, c.t, 0);
            if (rc) return rc;
        }
        return MPFFT_OK;
    }

    PairArgs pair_args(int op, long off, long h, long i0, long cnt, u64 rho) const
    {
        PairArgs a;
        memset(&a, 0, sizeof(a));
        a.dig = col.dig[0];
        a.cb = col.cb[0];
        a.top = col.top[0];
        a.N = P.N;
        a.l = (int)P.l;
        a.op = op;
        a.NC = ccount;
        a.ncol = ccount;
        a.off = (int)off;
        a.h = (int)h;
        a.i0 = (int)i0;
        a.cnt = (int)cnt;
        a.rho = rho;
        return a;
    }

    int pairop(int op, long off, long h, long i0, long cnt, u64 rho)
    {
        if (cnt <= 0) return MPFFT_OK;
        int rc;
        const bool chains = P.rpass && rp_chain_get((int)P.l, 1) && !diag_env("MPFFT_NO_CHAIN");
        if (chains && op == OP_TWOXMY && i0 == 0) {
            if (chain.n && (chain.off != off || chain.t != cnt || chain.n == 3) && (rc = flush_chain())) return rc;
            if (!chain.n) {
                chain.off = off;
                chain.t = cnt;
            }
            chain.h[chain.n++] = h;
            return MPFFT_OK;
        }
        if (chains && op == OP_IBFLY && i0 == 0 && chain.n && chain.off == off + h && chain.t == cnt) {
            PairArgs a = pair_args(op, off + h, h, 0, cnt, rho);
            a.nb = chain.n;
            for (int j = 0; j < chain.n; ++j) a.hb[j] = (int)chain.h[j];
            a.xoff = (int)off;
            rp_pair_fn f = rp_chain_get((int)P.l, chain.n);
            chain.n = 0;
            if (rec) {
                char ln[96];
                snprintf(ln, sizeof ln, "k_rchain<%d,%d> off=%ld h=%ld cnt=%ld\n", (int)P.l / 1024, a.nb, off + h, h, cnt);
                *rec += ln;
                return MPFFT_OK;
            }
            return launch(f, dim3((unsigned)(cnt * ccount)), dim3(RP_NT), rp_chain_lds((int)P.l), a);
        }
        if ((rc = flush_chain())) return rc;
        return pairop_now(op, off, h, i0, cnt, rho);
    }

    int pairop_now(int op, long off, long h, long i0, long cnt, u64 rho)
    {
        if (cnt <= 0) return MPFFT_OK;
        if (rec) {
            char ln[96];
            if (P.rpass) snprintf(ln, sizeof ln, "k_rpair<%d,%d> off=%ld h=%ld i0=%ld cnt=%ld\n", (int)P.l / 1024, op, off, h, i0, cnt);
            else snprintf(ln, sizeof ln, "pair<%d> off=%ld h=%ld i0=%ld cnt=%ld\n", op, off, h, i0, cnt);
            *rec += ln;
            return MPFFT_OK;
        }
        const PairArgs a = pair_args(op, off, h, i0, cnt, rho);
        const long pairs = cnt * ccount;
        if (P.rpass) {   // register-resident pair steps (rkernels.hpp)
            rp_pair_fn f = rp_pair_get((int)P.l, op);
            if (!f) return MPFFT_EUNSUPPORTED;
            return launch(f, dim3((unsigned)pairs), dim3(RP_NT), rp_pair_lds((int)P.l), a);
        }
        if (P.wave)   // a wave per pair
            return launch(wv_fns(P.wU, P.wfull).pair, dim3((unsigned)((pairs + WPB - 1) / WPB)), dim3(64 * WPB),
                          (size_t)WPB * 16 * P.l, a);
        void (*f)(PairArgs) = nullptr;
        switch (P.U) {
        case 1: f = k_pairop<1>; break;
        case 2: f = k_pairop<2>; break;
        case 4: f = k_pairop<4>; break;
        }
        return launch(f, dim3((unsigned)pairs), dim3(P.tpb), lds_bytes((int)P.l, 2, 2, P.U, nw), a);
    }

    u64 rho_blk(long m) const { return (u64)P.w * P.NC * (u64)(P.NR / m); }

    // IFFT_radix2_truncate(_twiddle) (mul_fft.c:1733-1790): outputs [off, off+t) known,
    // inputs >= t zero; root of a length-m block = 2^(w NC NR/m)
    // public entries: the recursion, then whatever it left in the chain
    int itft(long off, long m, long t)
    {
        int rc = itft_r(off, m, t);
        return rc ? rc : flush_chain();
    }
    int itft1(long off, long m, long t)
    {
        int rc = itft1_r(off, m, t);
        return rc ? rc : flush_chain();
    }

    int itft_r(long off, long m, long t)
    {
        int rc;
        const long h = m / 2;
        const bool top = defer_double && off == 0 && m == P.NR;   // its doubling folds into the scaling
        if (t == m) return ifft_block(off, m);
        if (t <= h) {
            if ((rc = itft_r(off, h, t))) return rc;
            if (top) {
                dbl_lo = 0;
                dbl_hi = t;
                return MPFFT_OK;
            }
            return pairop(OP_DOUBLE, off, h, 0, t, 0);
        }
        // itft1_r(off + h, h, t - h) below half-adds at the distances h/2, h/4, .. while t - h is below them
        long hmin = 0;
        if (tail_fold)
            for (long d = h / 2; d > t - h; d /= 2) hmin = d;
        fill = {t - h, h, rho_blk(m), false, hmin, 0};   // offered to ifft_block's last pass
        rc = ifft_block(off, h);
        const bool filled = fill.done;
        const long habs = fill.habs;
        fill = {};
        if (rc) return rc;
        if (!filled && (rc = pairop(OP_FILL, off, h, t - h, h - (t - h), rho_blk(m)))) return rc;
        if ((rc = itft1_r(off + h, h, t - h, habs))) return rc;
        if ((rc = pairop(OP_IBFLY, off, h, 0, t - h, rho_blk(m)))) return rc;
        if (top) {
            dbl_lo = t - h;
            dbl_hi = h;
            return MPFFT_OK;
        }
        return pairop(OP_DOUBLE, off, h, t - h, h - (t - h), 0);
    }

    // IFFT_radix2_truncate1(_twiddle) (mul_fft.c:1604-1668): inputs [t, m) known
    // habs: the FILL pass before it has done the half-adds of distance >= habs (0: none); the
    // blocks only shrink from here on, so those are the ones at the head of this recursion
    int itft1_r(long off, long m, long t, long habs = 0)
    {
        int rc;
        const long h = m / 2;
        if (t == m) return ifft_block(off, m);
        if (t <= h) {
            if (!(habs && h >= habs) && (rc = pairop(OP_HALFADD, off, h, t, h - t, 0))) return rc;
            if ((rc = itft1_r(off, h, t, habs))) return rc;
            return pairop(OP_TWOXMY, off, h, 0, t, 0);
        }
        if ((rc = ifft_block(off, h))) return rc;
        if ((rc = pairop(OP_FIX, off, h, t - h, h - (t - h), rho_blk(m)))) return rc;
        if ((rc = itft1_r(off + h, h, t - h))) return rc;
        return pairop(OP_IBFLY, off, h, 0, t - h, rho_blk(m));
    }

    // scaling by 2^-(depth+1); rows [dbl_lo, dbl_hi) by 2^-depth (itft's deferred doubling)
    int scale()
    {
        if (P.fuse_scale || fold) return MPFFT_OK;   // done by the last inverse column / row pass
        const u64 e = 2 * P.N - (u64)(P.depth + 1);
        if (dbl_hi <= dbl_lo) return scale_rows(0, P.Tr, e);
        if (P.rpass) return scale_rows(0, P.Tr, e, dbl_lo, dbl_hi);   // one launch, two exponents
        int rc;
        if ((rc = scale_rows(0, dbl_lo, e))) return rc;
        if ((rc = scale_rows(dbl_lo, dbl_hi, e + 1))) return rc;
        return scale_rows(dbl_hi, P.Tr, e);
    }

    // rows [r0_, r1_) by 2^e; with rpass, rows [d0, d1) inside them by 2^(e+1), and slot j of
    // the launch by 2^(e - j estep) (estep != 0: unweight())
    int scale_rows(long r0_, long r1_, u64 e, long d0 = 0, long d1 = 0, u64 estep = 0)
    {
        const long cnt = (r1_ - r0_) * ccount, s0 = r0_ * ccount;
        if (cnt <= 0) return MPFFT_OK;
        View v = col;
        v.advance(s0, P.l);
        u64 *dig = v.dig[0], *cbp = v.cb[0];
        int *top = v.top[0];
        if (P.rpass) {   // register-resident scale + canonicalisation (rkernels.hpp)
            // threads per coefficient: 256 up to l = 2048 (C3 scale 0.36 -> 0.31 ms: more coefficients
            // in flight per CU), 512 at l = 4096 (C4 2.61 vs 2.96 ms: the canonical sweep's rows per
            // wave double); profiles/r03/scale_nt_ab.txt
            static const int snt_env = [] { const char *e = diag_env("MPFFT_SCALE_NT"); return e ? atoi(e) : 0; }();
            const int snt = snt_env == 256 || snt_env == 512 ? snt_env : P.l <= 2048 ? 256 : 512;
            rp_scale_fn f = rp_scale_get((int)P.l, snt);
            if (!f) return MPFFT_EUNSUPPORTED;
            const unsigned lo = (unsigned)((d0 - r0_) * ccount), hi = (unsigned)((d1 - r0_) * ccount);
            return launch(f, dim3((unsigned)cnt), dim3(snt), rp_scale_lds((int)P.l), dig, cbp, top, (unsigned)P.N,
                          (unsigned)e, (unsigned)(e + 1), d1 > d0 ? lo : 0u, d1 > d0 ? hi : 0u, (unsigned)estep);
        }
        if (estep) return MPFFT_EINVAL;   // the per-slot exponent is k_rscale's alone
        if (P.wave)
            return launch(wv_fns(P.wU, P.wfull).scale, dim3((unsigned)((cnt + WPB - 1) / WPB)), dim3(64 * WPB),
                          (size_t)WPB * 16 * P.l, dig, cbp, top, (int)P.l, P.N, e, cnt);
        void (*f)(u64 *, u64 *, int *, int, u64, u64) = nullptr;
        switch (P.U) {
        case 1: f = k_scale<1>; break;
        case 2: f = k_scale<2>; break;
        case 4: f = k_scale<4>; break;
        }
        return launch(f, dim3((unsigned)cnt), dim3(P.tpb), lds_bytes((int)P.l, 1, 1, P.U, nw), dig, cbp, top, (int)P.l, P.N, e);
    }

    // combine stripes (combine.hpp): `a` names the coefficients, the stripes (a.G, a.g, a.S, a.C)
    // and the halo; nst stripes of this launch, each comb_blocks(stripe limbs) blocks, in one
    // k_combine1 launch (window sums plus a per-stripe decoupled look-back carry chain, carry-in
    // 0).  st: the look-back flags (nst bps + 1 u32, zeroed here unless `cleared`); allp (or
    // null): per-block all-ones flags for the stripe summaries.
    int combine1(CombArgs a, long nst, long stripe_limbs, u64 *r, u32 *st, bool cleared, u32 *allp)
    {
        a.l = (int)P.l;
        a.N = P.N;
        a.bits1 = P.bits1;
        a.len = P.len;
        a.total = P.total;
        a.inv_bits1 = 1.0 / (double)P.bits1;
        a.bps = comb_blocks(P, stripe_limbs);
        const long nb = nst * a.bps;
        if (!cleared) HIPCHK(hipMemsetAsync(st, 0, (size_t)(nb + 1) * 4, s));   // one fill
        const int v = comb_v();
        const bool k3 = (P.N + 63 + P.bits1 - 1) / P.bits1 <= 3;   // at most 3 coefficients cover a limb
        void (*f)(CombArgs, u64 *, u32 *, u32 *) =
            k3 ? (v == 1 ? k_combine1<1, 3> : v == 2 ? k_combine1<2, 3> : v == 4 ? k_combine1<4, 3>
                  : v == 16 ? k_combine1<16, 3> : k_combine1<8, 3>)
               : (v == 1 ? k_combine1<1, 0> : v == 2 ? k_combine1<2, 0> : v == 4 ? k_combine1<4, 0>
                  : v == 16 ? k_combine1<16, 0> : k_combine1<8, 0>);
        // consecutive limbs per thread: the wave's pairs loaded coalesced and handed out through LDS
        // (C3 combine 0.300 -> 0.285 ms against per-lane pair loads; MPFFT_COMB_XP = 0 for A/B)
        static const bool no_xp = [] { const char *e = diag_env("MPFFT_COMB_XP"); return e && !strcmp(e, "0"); }();
        const int nt = comb_nt(P);
        if (comb_ct(P)) {
            const bool k3w = comb_kw(P) <= 3;
            if (!no_xp) f = nt == 512 ? (k3w ? k_combine1<8, 3, true, 512, true> : k_combine1<8, 4, true, 512, true>)
                                      : (k3w ? k_combine1<8, 3, true, 256, true> : k_combine1<8, 4, true, 256, true>);
            else f = nt == 512 ? (k3w ? k_combine1<8, 3, true, 512> : k_combine1<8, 4, true, 512>)
                               : (k3w ? k_combine1<8, 3, true> : k_combine1<8, 4, true>);
        }
        return launch(f, dim3((unsigned)nb), dim3(nt), 0, a, r, st, allp);   // st[nb]: the ticket counter
    }

    // f4: the combine from the reduced form (fold.hpp): k_cmeta, then k_combine_red; rows
    // [lo, hi) of the coefficients doubled
    int combine_fold(u64 *r, unsigned char *ws, long lo, long hi)
    {
        FoldArgs a;
        memset(&a, 0, sizeof(a));
        a.dig = row.dig[0];
        a.cb = row.cb[0];
        a.top = row.top[0];
        a.meta = (int *)(ws + P.off_meta);
        a.l = (int)P.l;
        a.cbw = cb_words((int)P.l);
        a.N = P.N;
        a.bits1 = P.bits1;
        a.len = P.len;
        a.total = P.total;
        a.lbC = P.lbC;
        a.dbl_lo = (int)lo;
        a.dbl_hi = (int)hi;
        a.inv_bits1 = 1.0 / (double)P.bits1;
        constexpr int NT = 512;
        a.bps = (P.total + 8 * NT - 1) / (8 * NT);
        u32 *st = comb_flags(ws);
        if (zflags != st) HIPCHK(hipMemsetAsync(st, 0, (size_t)(a.bps + 1) * 4, s));
        auto cm = P.l == 1024 ? k_cmeta<16> : P.l == 2048 ? k_cmeta<32> : P.l == 4096 ? k_cmeta<64> : k_cmeta<0>;
        if (int rc = launch(cm, dim3((unsigned)((P.len + 255) / 256)), dim3(256), 0, a)) return rc;   // a lane per coefficient
        void (*f)(FoldArgs, u64 *, u32 *) = P.fold == 3 ? k_combine_red<3, NT> : k_combine_red<4, NT>;
        // persistent grid: the resident block count (workgroups take tickets until none are left)
        long grid = a.bps;
        int per = 0, ncu = 0, dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess
            && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void *)f, NT, 0) == hipSuccess && per > 0 && ncu > 0)
            grid = std::min<long>(grid, (long)per * ncu);
        return launch(f, dim3((unsigned)grid), dim3(NT), 0, a, r, st);
    }

    // one GPU: a single stripe over the natural slot order (coefficient k at slot k)
    int combine_single(u64 *r, unsigned char *ws)
    {
        u32 *st = comb_flags(ws);
        CombArgs a;
        memset(&a, 0, sizeof(a));
        a.dig = row.dig[0];
        a.C = P.trunc;
        a.G = 1;
        a.S = 1;
        return combine1(a, 1, P.total, r, st, zflags == st, nullptr);
    }

    // ---- the negacyclic top level (nega.hpp) on a make_plan_mod plan ----------------------
    // the shape of its slot-wise kernels, as the sqrt2 top level's: l = 2048 runs four limbs per
    // thread over 512 threads (two over 1024 spill)
    int nega_u() const { return P.U == 2 && P.l == 2048 ? 4 : P.U; }
    int nega_tpb() const { return nega_u() != P.U ? 512 : P.tpb; }
    size_t nega_lds() const { return lds_bytes((int)P.l, s2_rb(nega_u()), 3, nega_u(), nega_tpb() / 64); }

    NegaArgs nega_args() const
    {
        NegaArgs a;
        memset(&a, 0, sizeof(a));
        for (int k = 0; k < 2; ++k) {
            a.dig[k] = col.dig[k];
            a.cb[k] = col.cb[k];
            a.top[k] = col.top[k];
        }
        a.L = P.n1;
        a.bits1 = P.bits1;
        a.N = P.N;
        a.w = (u64)P.w;
        a.l = (int)P.l;
        a.depth = P.depth;
        return a;
    }

    // words of both combine flag regions from comb_flags() on (the weight launch clears them)
    static long nega_flag_words(const Plan &P) { return (long)((P.off_nflags - P.off_flags) / 4) + nega_blocks(P.n1) + 2; }

    // split + weight: slot j <- theta^j piece j of each operand (nops 1: operand 0 alone)
    int nweight(const u64 *srcA, const u64 *srcB, int nops)
    {
        NegaArgs a = nega_args();
        a.src[0] = srcA;
        a.src[1] = srcB;
        a.zp = zflags;
        a.zn = zflags_n;
        void (*f)(NegaArgs) = nullptr;
        switch (nega_u()) {
        case 1: f = k_nweight<1>; break;
        case 2: f = k_nweight<2>; break;
        case 4: f = k_nweight<4>; break;
        }
        if (!f) return MPFFT_EUNSUPPORTED;
        return launch(f, dim3((unsigned)(2 * P.n), (unsigned)nops), dim3(nega_tpb()), nega_lds(), a);
    }

    // un-weight + scaling: slot j <- theta^-j 2^-(depth+1) slot j, canonical.  Register-pass
    // plans with even w: k_rscale with the exponent taken from the slot index; else k_nunweight
    bool unweight_rscale() const { return P.rpass && P.w % 2 == 0; }
    int unweight()
    {
        if (unweight_rscale()) return scale_rows(0, P.NR, 2 * P.N - (u64)(P.depth + 1), 0, 0, (u64)P.w / 2);
        const NegaArgs a = nega_args();
        void (*f)(NegaArgs) = nullptr;
        switch (nega_u()) {
        case 1: f = k_nunweight<1>; break;
        case 2: f = k_nunweight<2>; break;
        case 4: f = k_nunweight<4>; break;
        }
        if (!f) return MPFFT_EUNSUPPORTED;
        return launch(f, dim3((unsigned)(2 * P.n)), dim3(nega_tpb()), nega_lds(), a);
    }

    // negacyclic combine: k_combine1 into the scratch, k_nwrap, k_nfix; r: L + 1 limbs
    int ncombine(u64 *r, unsigned char *ws)
    {
        u64 *T = (u64 *)(ws + P.off_nscr);
        u32 *st = (u32 *)(ws + P.off_nflags);
        const bool cleared = zflags == comb_flags(ws);
        int rc = combine_single(T, ws);
        if (rc) return rc;
        NegaCombArgs a;
        memset(&a, 0, sizeof(a));
        a.T = T;
        a.TL = P.total;
        a.dig = row.dig[0];
        a.top = row.top[0];
        a.l = (int)P.l;
        a.N = P.N;
        a.bits1 = P.bits1;
        a.L = P.n1;
        a.len = P.len;
        a.nT = (int)((P.total + P.n1 - 1) / P.n1);
        a.qmax = (int)(((u64)(P.len - 1) * P.bits1 + P.N) / (64 * (u64)P.n1));
        a.K = 2u * (u32)(a.nT / 2 + 1 + a.qmax / 2 + 1);
        a.inv_bits1 = 1.0 / (double)P.bits1;
        a.nblk = nega_blocks(P.n1);
        if (!cleared) HIPCHK(hipMemsetAsync(st, 0, (size_t)(a.nblk + 2) * 4, s));
        if ((rc = launch(k_nwrap<NEGA_V>, dim3((unsigned)a.nblk), dim3(256), 0, a, r, st))) return rc;
        return launch(k_nfix, dim3(1), dim3(1024), 0, r, (long)P.n1, (const u32 *)st, a.nblk);
    }

    // ---- the low-word CRT family (negaw.hpp) on a make_plan_mod plan with Plan::lowcrt --------
    // d <- the negacyclic convolution mod 2^32 of the operands' piece low words (srcB == srcA: a square).
    // Enough workgroups to fill the device: the terms are split over blockIdx.y where the outputs alone
    // give fewer than LC_BLOCKS.
    int nlowconv(const u64 *srcA, const u64 *srcB, unsigned char *ws)
    {
        constexpr long LC_BLOCKS = 2048;
        LowConvArgs a;
        memset(&a, 0, sizeof(a));
        a.src[0] = srcA;
        a.src[1] = srcB;
        a.L = P.n1;
        a.bits1 = P.bits1;
        a.len = P.len;
        a.d = (u32 *)(ws + P.off_lowd);
        const long kt = (P.len + LC_TK - 1) / LC_TK, nch = (P.len + LC_TI - 1) / LC_TI;
        const long split = std::min(nch, std::max(1L, LC_BLOCKS / kt));
        a.ichunks = (int)((nch + split - 1) / split);
        const long gy = (nch + a.ichunks - 1) / a.ichunks;
        HIPCHK(hipMemsetAsync(a.d, 0, (size_t)P.len * 4, s));
        return launch(k_nlowconv, dim3((unsigned)kt, (unsigned)gy), dim3(LC_NT), 0, a);
    }

    // the fold with the low-word CRT: k_combine1 into the scratch, k_nwrapw (reads the canonical slots
    // and d), k_nfix; r: L + 1 limbs
    int ncombinew(u64 *r, unsigned char *ws)
    {
        u64 *T = (u64 *)(ws + P.off_nscr);
        u32 *st = (u32 *)(ws + P.off_nflags);
        const bool cleared = zflags == comb_flags(ws);
        int rc = combine_single(T, ws);
        if (rc) return rc;
        NegaWCombArgs aw;
        memset(&aw, 0, sizeof(aw));
        NegaCombArgs &a = aw.b;
        a.T = T;
        a.TL = P.total;
        a.dig = row.dig[0];
        a.top = row.top[0];
        a.l = (int)P.l;
        a.N = P.N;
        a.bits1 = P.bits1;
        a.L = P.n1;
        a.len = P.len;
        a.nT = (int)((P.total + P.n1 - 1) / P.n1);
        a.qmax = (int)(((u64)(P.len - 1) * P.bits1 + P.N + 31) / (64 * (u64)P.n1));
        // negative pieces: the odd T_i, C, the odd Wb_q and Eb_q, the even Cb_q
        a.K = 2u * (u32)(a.nT / 2 + 1 + 2 * ((a.qmax + 1) / 2) + a.qmax / 2 + 1);
        a.inv_bits1 = 1.0 / (double)P.bits1;
        a.nblk = nega_blocks(P.n1);
        aw.d = (const u32 *)(ws + P.off_lowd);
        if (!cleared) HIPCHK(hipMemsetAsync(st, 0, (size_t)(a.nblk + 2) * 4, s));
        if ((rc = launch(k_nwrapw<NEGA_V>, dim3((unsigned)a.nblk), dim3(256), 0, aw, r, st))) return rc;
        return launch(k_nfix, dim3(1), dim3(1024), 0, r, (long)P.n1, (const u32 *)st, a.nblk);
    }

    // ---- the cyclic top level (cyc.hpp) on a make_plan_cyc plan ---------------------------
    // words of both combine flag regions from comb_flags() on (the first forward column pass clears them)
    static long cyc_flag_words(const Plan &P) { return (long)((P.off_nflags - P.off_flags) / 4) + cyc_blocks(P.n1) + CYC_XW; }

    // the plain scaling by 2^-(depth+1), canonical, whatever the plan fuses (the stage entry)
    int cscale() { return scale_rows(0, P.NR, 2 * P.N - (u64)(P.depth + 1)); }

    // cyclic combine: k_combine1 into the scratch, k_cwrap, k_cfix; r: L limbs
    int ccombine(u64 *r, unsigned char *ws)
    {
        u64 *T = (u64 *)(ws + P.off_nscr);
        u32 *st = (u32 *)(ws + P.off_nflags);
        const bool cleared = zflags == comb_flags(ws);
        int rc = combine_single(T, ws);
        if (rc) return rc;
        CycCombArgs a;
        memset(&a, 0, sizeof(a));
        a.T = T;
        a.TL = P.total;
        a.L = P.n1;
        a.nT = (int)((P.total + P.n1 - 1) / P.n1);
        a.nblk = cyc_blocks(P.n1);
        if (!cleared) HIPCHK(hipMemsetAsync(st, 0, (size_t)(a.nblk + CYC_XW) * 4, s));
        if ((rc = launch(k_cwrap<CYC_V>, dim3((unsigned)a.nblk), dim3(256), 0, a, r, st))) return rc;
        return launch(k_cfix, dim3(1), dim3(1024), 0, r, (long)P.n1, (const u32 *)st, a.nblk);
    }
};
