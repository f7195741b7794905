// Host-side unit test of pw_combine's grouped forms (mpir-fft_amd/csrc/pkernels.hpp, GRP): one wrap
// test, base select and mask select per two consecutive partner words, the word past the wrap
// read from row 2M (the complement of row 0) of the partner's column.  It must return
// bit-identical L, T, S to the per-word pw_combine<M, LK> on the same buffer -- rows 0 .. 2M-1
// the partner's words, row 2M their ~word0, everything else random -- for M = 10 and 18 at
// LK = 8 (the shapes k_pwss / k_pwsq run it at).  One case publishes a wrong row 2M and must
// differ: the row is used.  The same for the groups of four (the shipped K = 256 form, pw_group), on a
// buffer whose rows 2M .. 2M+2 hold ~word0 .. ~word2.
// Built by __graft_entry__.build() (tests/pw_pair_host/Makefile), run by tests/test_pw_pair_host.py.
#include "pkernels.hpp"
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>

static std::mt19937_64 rng(12);

enum { PAT_ZERO, PAT_ONES, PAT_W0_ZERO_W1_ONES, PAT_W0_ONES_W1_ZERO, PAT_RANDOM, NPAT };

template <int M> struct Case {
    static constexpr int LK = 8, K = 1 << LK, NW = 2 * M;
    std::vector<u32> Xw;
    Case() : Xw((size_t)(NW + 4) * K) { scramble(); }
    void scramble()
    {
        for (auto &w : Xw) w = (u32)rng();
    }
    // the partner's column q in the published layout; the rest of the buffer stays random
    // quad: rows 2M + 1, 2M + 2 = ~word1, ~word2 as well (left random otherwise: GRP = 2 must not read them)
    void fill(int q, int pat, bool wrong_row = false, bool quad = false)
    {
        for (int k = 0; k < NW; ++k) {
            u32 w = (u32)rng();
            if (pat == PAT_ZERO) w = 0;
            if (pat == PAT_ONES) w = ~0u;
            if (pat == PAT_W0_ZERO_W1_ONES && k < 2) w = k == 0 ? 0u : ~0u;
            if (pat == PAT_W0_ONES_W1_ZERO && k < 2) w = k == 0 ? ~0u : 0u;
            Xw[(size_t)k * K + q] = w;
        }
        Xw[(size_t)NW * K + q] = wrong_row ? Xw[q] : ~Xw[q];
        if (quad) {
            Xw[(size_t)(NW + 1) * K + q] = ~Xw[(size_t)K + q];
            Xw[(size_t)(NW + 2) * K + q] = wrong_row ? Xw[(size_t)2 * K + q] : ~Xw[(size_t)2 * K + q];
        }
    }
    // 0: both forms agree; 1: they differ
    template <int GRP = 2>
    int run(int q, unsigned E, int alpha, int S, int Sq, int Tq)
    {
        u64 L0[M], L1[M];
        for (int j = 0; j < M; ++j) L0[j] = L1[j] = rng();
        int T0 = (int)(rng() % 9) - 4, T1 = T0, S0 = S, S1 = S;
        const int packed = 2 * Tq + Sq;
        pw_combine<M, LK>(L0, T0, S0, alpha, Xw.data(), packed, q, E);
        pw_combine<M, LK, 2 * M, -1, GRP>(L1, T1, S1, alpha, Xw.data(), packed, q, E);
        return T0 != T1 || S0 != S1 || memcmp(L0, L1, sizeof L0) != 0;
    }
    // the same with the 128-VGPR kernels' prefetch distance (pw_pd: the same reads in another order)
    template <int GRP = 2>
    int run_pd(int q, unsigned E, int alpha, int S, int Sq, int Tq)
    {
        u64 L0[M], L1[M];
        for (int j = 0; j < M; ++j) L0[j] = L1[j] = rng();
        int T0 = (int)(rng() % 9) - 4, T1 = T0, S0 = S, S1 = S;
        const int packed = 2 * Tq + Sq;
        pw_combine<M, LK>(L0, T0, S0, alpha, Xw.data(), packed, q, E);
        pw_combine<M, LK, 16, -1, GRP>(L1, T1, S1, alpha, Xw.data(), packed, q, E);
        return T0 != T1 || S0 != S1 || memcmp(L0, L1, sizeof L0) != 0;
    }
};

static const int TQS[4] = {-1, 0, -2, 1};

// every sign combination, alpha and Tq at rotation E, for every partner pattern
template <int M> long sweep_full(Case<M> &c, unsigned E, long &n)
{
    long bad = 0;
    c.scramble();
    for (int pat = 0; pat < NPAT; ++pat) {
        const int q = (int)(rng() % Case<M>::K);
        c.fill(q, pat);
        for (int S = 0; S < 2; ++S)
            for (int Sq = 0; Sq < 2; ++Sq)
                for (int alpha = -1; alpha <= 1; ++alpha)
                    for (int Tq : TQS) {
                        const int d = c.run(q, E, alpha, S, Sq, Tq) | c.run_pd(q, E, alpha, S, Sq, Tq);
                        if (d && bad++ < 5) printf("M=%d mismatch E=%u pat=%d S=%d Sq=%d alpha=%d Tq=%d\n", M, E, pat, S, Sq, alpha, Tq);
                        ++n;
                    }
    }
    return bad;
}

template <int M> long run()
{
    constexpr unsigned NP = 64 * M, N2 = 2 * NP;
    constexpr int NW = 2 * M;
    Case<M> c;
    long bad = 0, n = 0;
    if (M == 10) {
        for (unsigned E = 0; E < N2; ++E) bad += sweep_full<M>(c, E, n);
    } else {
        // Yw = ((E mod N') - 1) >> 5 in {-1, 0, 1, 2M-2, 2M-1}; E == 0 or 31 mod 32; 10^4 random E
        for (unsigned E = 0; E < N2; ++E) {
            const int Yw = ((int)(E % NP) - 1) >> 5;
            const bool edge = Yw == -1 || Yw == 0 || Yw == 1 || Yw == NW - 2 || Yw == NW - 1;
            if (edge || E % 32 == 0 || E % 32 == 31) bad += sweep_full<M>(c, E, n);
        }
        for (int it = 0; it < 10000; ++it) {
            const unsigned E = (unsigned)(rng() % N2);
            if (it % 64 == 0) c.scramble();
            for (int pat = 0; pat < NPAT; ++pat) {
                const int q = (int)(rng() % Case<M>::K);
                c.fill(q, pat);
                const int alpha = (int)(rng() % 3) - 1, S = (int)(rng() & 1), Sq = (int)(rng() & 1), Tq = TQS[rng() % 4];
                const int d = c.run(q, E, alpha, S, Sq, Tq) | c.run_pd(q, E, alpha, S, Sq, Tq);
                if (d && bad++ < 5) printf("M=%d mismatch (random) E=%u pat=%d S=%d Sq=%d alpha=%d Tq=%d\n", M, E, pat, S, Sq, alpha, Tq);
                ++n;
            }
        }
    }
    // a wrong row 2M (word0 itself, not its complement) at a rotation whose wrap falls inside a
    // pair (Yw odd: words Yw - 1, Yw share the test): the paired form must differ from the per-word one
    long unused = 0;
    for (int Yw = 1; Yw < NW; Yw += 2) {
        const unsigned E = (unsigned)(32 * Yw + 1 + (int)(rng() % 32));
        const int q = (int)(rng() % Case<M>::K);
        c.fill(q, PAT_RANDOM, true);
        if (!c.run(q, E, 1, 0, 0, -1)) {
            ++unused;
            printf("M=%d wrong row 2M not noticed at E=%u\n", M, E);
        }
    }
    printf("M=%d pair combine cases=%ld bad=%ld wrong_row_unnoticed=%ld\n", M, n, bad, unused);
    // groups of four: every rotation, every pattern, random signs, alpha and partner top; then wrong
    // rows 2M and 2M + 2 at every odd Yw (the wrap then leaves word 0 inside a group)
    long bad4 = 0, unused4 = 0, n4 = 0;
    for (unsigned E = 0; E < N2; ++E)
        for (int pat = 0; pat < NPAT; ++pat) {
            const int q = (int)(rng() % Case<M>::K);
            c.fill(q, pat, false, true);
            const int alpha = (int)(rng() % 3) - 1, S = (int)(rng() & 1), Sq = (int)(rng() & 1), Tq = TQS[rng() % 4];
            const int d = c.template run<4>(q, E, alpha, S, Sq, Tq) | c.template run_pd<4>(q, E, alpha, S, Sq, Tq);
            if (d && bad4++ < 5) printf("M=%d quad mismatch E=%u pat=%d S=%d Sq=%d alpha=%d Tq=%d\n", M, E, pat, S, Sq, alpha, Tq);
            ++n4;
        }
    for (int Yw = 1; Yw < NW; Yw += 2) {
        const unsigned E = (unsigned)(32 * Yw + 1 + (int)(rng() % 32));
        const int q = (int)(rng() % Case<M>::K);
        c.fill(q, PAT_RANDOM, true, true);
        if (!c.template run<4>(q, E, 1, 0, 0, -1)) {
            ++unused4;
            printf("M=%d wrong rows 2M, 2M + 2 not noticed by the groups of four at E=%u\n", M, E);
        }
    }
    printf("M=%d quad combine cases=%ld bad=%ld wrong_row_unnoticed=%ld\n", M, n4, bad4, unused4);
    return bad + unused + bad4 + unused4;
}

int main()
{
    const long bad = run<10>() + run<18>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
