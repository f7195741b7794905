// Host-side unit test of the squaring kernel's inner product (mpir-fft_amd/csrc/pkernels.hpp):
// pw_sqrmod<M> against pw_mulmod<M>(a, a) and against GMP, for every inner size the library
// instantiates (M = 10, 18, 20), on the edge residues and on seeded random ones.  The same
// source runs on the GPU inside k_pwsq.  Stand-alone (own main), so it can also be built with
// -fsanitize=address,undefined and run directly.
// Built by __graft_entry__.build() (tests/pw_sqr_host/Makefile), run by tests/test_pw_sqr_host.py.
#include "pkernels.hpp"
#include <gmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
static std::mt19937_64 rng(11);
template <int M> void tovals(mpz_t z, const u64 *L, int T) {
    mpz_import(z, M, -1, 8, 0, 0, L);
    mpz_t t; mpz_init_set_si(t, T); mpz_mul_2exp(t, t, 64 * M); mpz_add(z, z, t); mpz_clear(t);
}
// one canonical residue (La, ta): the square against GMP and against pw_mulmod(a, a)
template <int M> int check(const u64 (&La)[M], int ta, const char *what, mpz_t p) {
    mpz_t a, want, got; mpz_inits(a, want, got, NULL);
    u64 Z[M], Zm[M]; int T = 99, Tm = 99;
    tovals<M>(a, La, ta); mpz_mul(want, a, a); mpz_mod(want, want, p);
    pw_sqrmod<M>(Z, T, La, ta);
    pw_mulmod<M>(Zm, Tm, La, ta, La, ta);
    int bad = 0;
    tovals<M>(got, Z, T); mpz_mod(got, got, p);
    if (mpz_cmp(got, want)) { printf("M=%d %s: sqrmod differs from GMP\n", M, what); ++bad; }
    tovals<M>(got, Zm, Tm); mpz_mod(got, got, p);
    if (mpz_cmp(got, want)) { printf("M=%d %s: mulmod(a, a) differs from GMP\n", M, what); ++bad; }
    // the same representative too: both stream the same columns through the same fold
    if (T != Tm || memcmp(Z, Zm, sizeof Z)) { printf("M=%d %s: sqrmod and mulmod(a, a) differ in limbs / top\n", M, what); ++bad; }
    if (T < -1 || T > 0) { printf("M=%d %s: top %d outside {-1, 0}\n", M, what, T); ++bad; }
    mpz_clears(a, want, got, NULL);
    return bad;
}
template <int M> int run() {
    mpz_t p; mpz_init(p);
    mpz_set_ui(p, 1); mpz_mul_2exp(p, p, 64 * M); mpz_add_ui(p, p, 1);
    int bad = 0;
    u64 L[M];
    for (int j = 0; j < M; ++j) L[j] = 0;
    bad += check<M>(L, 0, "0", p);
    L[0] = 1;
    bad += check<M>(L, 0, "1", p);
    for (int j = 0; j < M; ++j) L[j] = ~0ull;
    bad += check<M>(L, 0, "2^N' - 1", p);
    for (int j = 0; j < M; ++j) L[j] = 0;
    bad += check<M>(L, 1, "2^N' (ta = 1)", p);
    {   // ta = 1 gives exactly 1
        u64 Z[M]; int T = 5;
        pw_sqrmod<M>(Z, T, L, 1);
        bool one = T == 0 && Z[0] == 1;
        for (int j = 1; j < M; ++j) one = one && Z[j] == 0;
        if (!one) { printf("M=%d: (2^N')^2 is not the value 1\n", M); ++bad; }
    }
    for (int j = 0; j < M; ++j) L[j] = 0x8080808080808080ull;
    bad += check<M>(L, 0, "0x80 bytes", p);
    for (int j = 0; j < M; ++j) L[j] = 0x7f7f7f7f7f7f7f7full;
    bad += check<M>(L, 0, "0x7f bytes", p);
    {   // every 29-bit digit all ones: each column sum at its bound.  The top digit holds the
        // 64 M mod 29 bits that are left, so this is 2^N' - 1 when 29 does not divide 64 M; the
        // digits are also saturated one at a time below
        constexpr int DB = 29, ND = (64 * M + DB - 1) / DB;
        for (int j = 0; j < M; ++j) L[j] = ~0ull;
        bad += check<M>(L, 0, "all digits saturated", p);
        for (int d = 0; d < ND; ++d) {   // all ones except digit d, and digit d alone
            u64 A[M], B[M];
            for (int j = 0; j < M; ++j) { A[j] = ~0ull; B[j] = 0; }
            for (int b = d * DB; b < (d + 1) * DB && b < 64 * M; ++b) {
                A[b >> 6] &= ~(1ull << (b & 63));
                B[b >> 6] |= 1ull << (b & 63);
            }
            bad += check<M>(A, 0, "saturated but one digit", p);
            bad += check<M>(B, 0, "one saturated digit", p);
        }
    }
    for (int it = 0; it < 2000; ++it) {
        for (int j = 0; j < M; ++j) L[j] = rng();
        if (it % 9 == 4) for (int j = M / 2; j < M; ++j) L[j] = it % 2 ? ~0ull : 0;   // half-empty / half-full
        bad += check<M>(L, 0, "random", p);
        if (bad > 20) break;
    }
    printf("M=%d sqrmod bad=%d\n", M, bad);
    mpz_clear(p);
    return bad;
}

int main()
{
    int bad = run<10>() + run<18>() + run<20>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
