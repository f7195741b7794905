// Host-side unit test of k_pwmm's inner accumulation (mpir-fft_amd/csrc/pkernels.hpp): sums of up to
// PW_MM_MAX signed products formed as the kernel forms them -- pw_mulmod<M> on canonical factors, then
// pw_mm_add with the product's sign -- against GMP mod 2^N' + 1, for every inner size the library
// instantiates (M = 10, 18, 20).  Both signs are covered here: the records k_pwsx writes always give a
// product the sign 0, so no GPU input reaches the subtraction.  Also checked: the accumulator's top
// stays in [-2 kk, 2 kk], and pw_canon takes it from there.
// Stand-alone (own main), so it can also be built with -fsanitize=address,undefined and run directly.
// Built by __graft_entry__.build() (tests/pw_mm_host/Makefile), run by tests/test_pw_mm_host.py.
#include "pkernels.hpp"
#include <gmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
static std::mt19937_64 rng(18);

template <int M> void tovals(mpz_t z, const u64 *L, int T) {
    mpz_import(z, M, -1, 8, 0, 0, L);
    mpz_t t; mpz_init_set_si(t, T); mpz_mul_2exp(t, t, 64 * M); mpz_add(z, z, t); mpz_clear(t);
}

// a canonical residue of one of eight kinds: limbs in [0, 2^N'), flag 1 for 2^N' (limbs 0)
template <int M> int residue(u64 (&L)[M], int kind) {
    for (int j = 0; j < M; ++j)
        L[j] = kind == 0 ? rng() : kind == 2 ? ~0ull : kind == 5 ? 0x8080808080808080ull : kind == 6 ? 0x7f7f7f7f7f7f7f7full : 0ull;
    if (kind == 4) L[0] = 1;
    if (kind == 7) { for (int j = 0; j < M; ++j) L[j] = ~0ull; L[0] -= rng() & 0xffff; }
    return kind == 1;
}

template <int M> int run() {
    int bad = 0, tmin = 0, tmax = 0;
    mpz_t p, want, got, a, b, pr;
    mpz_inits(p, want, got, a, b, pr, NULL);
    mpz_set_ui(p, 1); mpz_mul_2exp(p, p, 64 * M); mpz_add_ui(p, p, 1);
    for (int it = 0; it < 6000; ++it) {
        const int kk = 1 + (int)(rng() % PW_MM_MAX);
        // the first 4096 cases walk the kinds and the signs of two terms, the rest are random
        u64 Z[M];
        for (int j = 0; j < M; ++j) Z[j] = 0;
        int Tz = 0;
        mpz_set_ui(want, 0);
        for (int t = 0; t < kk; ++t) {
            u64 La[M], Lb[M], W[M];
            int Tw;
            const int ka = it < 4096 && t < 2 ? (it >> (6 * t)) & 7 : (int)(rng() % 8);
            const int kb = it < 4096 && t < 2 ? (it >> (6 * t + 3)) & 7 : (int)(rng() % 8);
            const int ca = residue<M>(La, ka), cb = residue<M>(Lb, kb);
            const bool neg = (rng() & 1) != 0;
            pw_mulmod<M>(W, Tw, La, ca, Lb, cb);
            pw_mm_add<M>(Z, Tz, W, Tw, neg);
            tovals<M>(a, La, ca); tovals<M>(b, Lb, cb);
            mpz_mul(pr, a, b);
            if (neg) mpz_sub(want, want, pr); else mpz_add(want, want, pr);
        }
        if (Tz < tmin) tmin = Tz;
        if (Tz > tmax) tmax = Tz;
        if (Tz < -2 * kk || Tz > 2 * kk) { if (bad < 5) printf("M=%d kk=%d top %d out of range\n", M, kk, Tz); ++bad; }
        mpz_mod(want, want, p);
        tovals<M>(got, Z, Tz);
        mpz_mod(got, got, p);
        if (mpz_cmp(got, want)) { if (bad < 5) printf("M=%d kk=%d it=%d: accumulated sum differs\n", M, kk, it); ++bad; }
        // ... and through pw_canon, as the inverse's end sees a small top
        u64 C[M];
        for (int j = 0; j < M; ++j) C[j] = Z[j];
        const int flag = pw_canon<M>(C, Tz);
        tovals<M>(got, C, flag);
        if (mpz_cmp(got, want)) { if (bad < 5) printf("M=%d kk=%d it=%d: pw_canon of top %d differs\n", M, kk, it, Tz); ++bad; }
    }
    printf("M=%d sums bad=%d tops in [%d, %d]\n", M, bad, tmin, tmax);
    mpz_clears(p, want, got, a, b, pr, NULL);
    return bad;
}

int main() {
    const int bad = run<10>() + run<18>() + run<20>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
