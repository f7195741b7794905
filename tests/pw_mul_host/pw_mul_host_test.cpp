// Host-side unit test of the pointwise inner product pw_mulmod (mpir-fft_amd/csrc/pkernels.hpp)
// against GMP mpz for M = 10, 18, 20, on the inputs where a Karatsuba split over the N'/2 halves
// can go wrong: equal halves, every order of the halves of both operands, a half of ones against
// a half of zeros, 2^N' - 1 squared (every column at its maximum), 0, 1, single bits at
// N'/2 - 1, N'/2 and N' - 1, saturated digits, the ta / tb flags (2^N'), and 20 000 random pairs.
// Checked: limbs + T 2^N' congruent to a b mod p' = 2^N' + 1, and T inside the documented bound
// {-1, 0}; and the recombination's last fold (pw_kara_fold) on words near 0 and near 2^N'.
// Built twice by tests/pw_mul_host/Makefile: with the shipped per-M switch
// (pw_mul_host_test) and with the Karatsuba path at every M (pw_mul_host_test_kara,
// -DPW_KARA_MASK=7).  Run by tests/test_pw_mul_host.py.
#include "pkernels.hpp"
#include <gmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
static std::mt19937_64 rng(20261);

template <int M> struct Val {
    u64 L[M];
    int t;   // 1: the value is 2^N' (limbs 0)
};

template <int M> void tovals(mpz_t z, const u64 *L, int T)
{
    mpz_import(z, M, -1, 8, 0, 0, L);
    mpz_t t;
    mpz_init_set_si(t, T);
    mpz_mul_2exp(t, t, 64 * M);
    mpz_add(z, z, t);
    mpz_clear(t);
}

template <int M> Val<M> from_halves(const u64 *lo, const u64 *hi)
{
    Val<M> v;
    v.t = 0;
    for (int j = 0; j < M / 2; ++j) {
        v.L[j] = lo[j];
        v.L[j + M / 2] = hi[j];
    }
    return v;
}

template <int M> Val<M> bit(int pos)
{
    Val<M> v;
    v.t = 0;
    for (int j = 0; j < M; ++j) v.L[j] = 0;
    v.L[pos >> 6] = 1ull << (pos & 63);
    return v;
}

template <int M> std::vector<Val<M>> specials()
{
    constexpr int H = M / 2;
    std::vector<Val<M>> s;
    u64 zero[H], ones[H], r1[H], r2[H], big[H], small[H];
    for (int j = 0; j < H; ++j) {
        zero[j] = 0;
        ones[j] = ~0ull;
        r1[j] = rng();
        r2[j] = rng();
        big[j] = rng() | (1ull << 63);
        small[j] = rng() >> 1;
    }
    small[H - 1] >>= 1;
    big[H - 1] |= 3ull << 62;
    s.push_back(from_halves<M>(zero, zero));           // 0
    s.push_back(bit<M>(0));                            // 1
    s.push_back(from_halves<M>(ones, ones));           // 2^N' - 1
    s.push_back(from_halves<M>(ones, zero));           // a half of ones against a half of zeros
    s.push_back(from_halves<M>(zero, ones));
    s.push_back(from_halves<M>(r1, r1));               // a0 == a1
    s.push_back(from_halves<M>(r2, r2));
    s.push_back(from_halves<M>(big, small));           // a0 > a1
    s.push_back(from_halves<M>(small, big));           // a0 < a1
    s.push_back(from_halves<M>(r1, r2));
    s.push_back(from_halves<M>(r2, r1));
    s.push_back(bit<M>(32 * M - 1));                   // single bits around the split and at the top
    s.push_back(bit<M>(32 * M));
    s.push_back(bit<M>(64 * M - 1));
    Val<M> top;                                        // 2^N'
    top.t = 1;
    for (int j = 0; j < M; ++j) top.L[j] = 0;
    s.push_back(top);
    Val<M> alt;                                        // 0x80 / 0x7f bytes
    alt.t = 0;
    for (int j = 0; j < M; ++j) alt.L[j] = 0x8080808080808080ull;
    s.push_back(alt);
    for (int j = 0; j < M; ++j) alt.L[j] = 0x7f7f7f7f7f7f7f7full;
    s.push_back(alt);
    return s;
}

template <int M> int run()
{
    mpz_t p, a, b, want, got;
    mpz_inits(p, a, b, want, got, NULL);
    mpz_set_ui(p, 1);
    mpz_mul_2exp(p, p, 64 * M);
    mpz_add_ui(p, p, 1);
    int bad = 0, tmin = 0, tmax = 0;
    auto check = [&](const Val<M> &x, const Val<M> &y, const char *what, int it) {
        u64 Z[M];
        int T = 12345;
        tovals<M>(a, x.L, x.t);
        tovals<M>(b, y.L, y.t);
        mpz_mul(want, a, b);
        mpz_mod(want, want, p);
        pw_mulmod<M>(Z, T, x.L, x.t, y.L, y.t);
        tovals<M>(got, Z, T);
        mpz_mod(got, got, p);
        if (mpz_cmp(got, want)) {
            if (bad++ < 5) printf("M=%d %s mismatch it=%d\n", M, what, it);
        }
        if (T < -1 || T > 0) {
            if (bad++ < 5) printf("M=%d %s top out of range T=%d it=%d\n", M, what, T, it);
        }
        tmin = T < tmin ? T : tmin;
        tmax = T > tmax ? T : tmax;
    };
    const std::vector<Val<M>> s = specials<M>();
    for (size_t i = 0; i < s.size(); ++i)
        for (size_t j = 0; j < s.size(); ++j) check(s[i], s[j], "special", (int)(i * 100 + j));
    for (int it = 0; it < 20000; ++it) {
        Val<M> x, y;
        x.t = y.t = 0;
        for (int j = 0; j < M; ++j) {
            x.L[j] = rng();
            y.L[j] = rng();
        }
        if (it % 16 == 1)   // sparse: long runs of zero digits
            for (int j = 0; j < M; ++j) {
                x.L[j] &= rng() & rng() & rng();
                y.L[j] &= rng() & rng();
            }
        if (it % 16 == 2)   // dense: long runs of one digits
            for (int j = 0; j < M; ++j) {
                x.L[j] |= rng() | rng() | rng();
                y.L[j] |= rng() | rng();
            }
        if (it % 16 == 3)   // halves that differ in their low limb only
            for (int j = 1; j < M / 2; ++j) {
                x.L[j + M / 2] = x.L[j];
                y.L[j + M / 2] = y.L[j];
            }
        check(x, y, "random", it);
        if (it % 64 == 5) check(x, s[it % s.size()], "random x special", it);
    }
    printf("M=%d kara=%d mulmod bad=%d top range [%d, %d]\n", M, (int)pw_kara<M>(), bad, tmin, tmax);
    mpz_clears(p, a, b, want, got, NULL);
    return bad;
}

// pw_kara_fold on its own: words near 0 and near 2^N' with every small (clo, chi), so that the
// chain's top reaches -1, 0 and 1 (the last one is the second fold, which products reach with
// probability ~2^-N'), plus random words; value and top range against GMP
template <int M> int run_fold()
{
    mpz_t p, want, got, t;
    mpz_inits(p, want, got, t, NULL);
    mpz_set_ui(p, 1);
    mpz_mul_2exp(p, p, 64 * M);
    mpz_add_ui(p, p, 1);
    int bad = 0, tops[3] = {0, 0, 0}, second = 0;
    for (int kind = 0; kind < 40; ++kind)
        for (int clo = -7; clo <= 7; ++clo)
            for (int chi = -7; chi <= 7; ++chi) {
                u32 Zw[2 * M];
                for (int k = 0; k < 2 * M; ++k) Zw[k] = kind < 16 ? 0u : kind < 32 ? ~0u : (u32)rng();
                if (kind < 32) Zw[0] = (kind < 16 ? 0u : ~0u) + (u32)(kind & 15) - 8u * (kind >= 16);
                if (kind >= 8 && kind < 16) for (int k = M; k < 2 * M; ++k) Zw[k] = ~0u;   // low half 0, high half ones
                if (kind >= 24 && kind < 32) for (int k = M; k < 2 * M; ++k) Zw[k] = 0u;
                mpz_import(want, 2 * M, -1, 4, 0, 0, Zw);
                mpz_set_si(t, clo); mpz_mul_2exp(t, t, 32 * M); mpz_add(want, want, t);
                mpz_set_si(t, chi); mpz_mul_2exp(t, t, 64 * M); mpz_add(want, want, t);
                // the first chain's sum Zw + clo X - chi reaches 2^N': the second fold runs
                mpz_import(got, 2 * M, -1, 4, 0, 0, Zw);
                mpz_set_si(t, clo); mpz_mul_2exp(t, t, 32 * M); mpz_add(got, got, t);
                mpz_set_si(t, chi); mpz_sub(got, got, t);
                mpz_sub_ui(t, p, 1);
                const bool big = mpz_cmp(got, t) >= 0;
                mpz_mod(want, want, p);
                const int top = pw_kara_fold<M>(Zw, clo, chi);
                mpz_import(got, 2 * M, -1, 4, 0, 0, Zw);
                mpz_set_si(t, top); mpz_mul_2exp(t, t, 64 * M); mpz_add(got, got, t);
                mpz_mod(got, got, p);
                if (mpz_cmp(got, want) || top < -1 || top > 0) {
                    if (bad++ < 5) printf("M=%d fold mismatch kind=%d clo=%d chi=%d top=%d\n", M, kind, clo, chi, top);
                }
                if (top >= -1 && top <= 0) ++tops[top + 1];
                second += big;
            }
    if (!second || !tops[0] || !tops[1]) { printf("M=%d fold: a case was never reached\n", M); ++bad; }
    printf("M=%d fold bad=%d tops -1: %d, 0: %d, second folds: %d\n", M, bad, tops[0], tops[1], second);
    mpz_clears(p, want, got, t, NULL);
    return bad;
}

int main()
{
    int bad = run<10>() + run<18>() + run<20>();
    bad += run_fold<10>() + run_fold<18>() + run_fold<20>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
