// Host-side unit test of the carry chains around the pointwise inner product
// (mpir-fft_amd/csrc/pkernels.hpp) against GMP mpz, for M = 10, 18, 20:
//   pw_canon:  the limbs are the residue of L - T mod p' = 2^N' + 1 in [0, 2^N'], the flag set
//              exactly for 2^N' (limbs 0 then);
//   pw_sqrt2:  L' + T' 2^N' == (2^(N'/2) - 1) (L + T 2^N') mod p', |T'| <= |T| + 3.
// Inputs: L = 0, 1, 2^N' - 1; a low word of 0 and of 0xffffffff under every T in -3 .. 3 (pw_canon's
// common path and its wrapped low word, both counted); all-ones halves, and for pw_sqrt2 the halves
// whose difference leaves the high half's low word at 0 .. 2 (the rippled carry, counted); 20 000
// random values.  Run by tests/test_pw_chain_host.py.
#include "pkernels.hpp"
#include <gmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>
static std::mt19937_64 rng(20271);

template <int M> struct Val {
    u64 L[M];
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

template <int M> Val<M> fill(u64 lo, u64 hi)
{
    Val<M> v;
    for (int j = 0; j < M; ++j) v.L[j] = j < M / 2 ? lo : hi;
    return v;
}

template <int M> std::vector<Val<M>> placed()
{
    std::vector<Val<M>> s;
    s.push_back(fill<M>(0, 0));                       // 0
    Val<M> v = fill<M>(0, 0);
    v.L[0] = 1;
    s.push_back(v);                                   // 1
    s.push_back(fill<M>(~0ull, ~0ull));               // 2^N' - 1
    s.push_back(fill<M>(~0ull, 0));                   // all-ones halves
    s.push_back(fill<M>(0, ~0ull));
    // low word 0 / 0xffffffff: below zeros, below ones, below random limbs
    for (int top = 0; top < 3; ++top)
        for (int lw = 0; lw < 2; ++lw) {
            Val<M> x;
            for (int j = 0; j < M; ++j) x.L[j] = top == 0 ? 0 : top == 1 ? ~0ull : rng();
            x.L[0] = (x.L[0] & ~0xffffffffull) | (lw ? 0xffffffffull : 0);
            s.push_back(x);
            x.L[0] = lw ? 0xffffffffull : 0;          // ... and the whole low limb
            s.push_back(x);
        }
    // equal halves but for a difference d in the low word: lo - hi - T small, T - hi - lo borrows
    for (int d = 0; d < 4; ++d) {
        Val<M> x;
        for (int j = 0; j < M / 2; ++j) x.L[j] = x.L[j + M / 2] = rng();
        x.L[0] = (x.L[M / 2] & ~0xffffffffull) | (u32)((u32)x.L[M / 2] + (u32)d);
        s.push_back(x);
        for (int j = 1; j < M / 2; ++j) x.L[j] = x.L[j + M / 2] = 0;   // ... the borrow runs through zeros
        s.push_back(x);
    }
    return s;
}

template <int M> int run()
{
    mpz_t p, half, x, want, got, lo, hi;
    mpz_inits(p, half, x, want, got, lo, hi, NULL);
    mpz_set_ui(p, 1);
    mpz_mul_2exp(p, p, 64 * M);
    mpz_add_ui(p, p, 1);
    mpz_set_ui(half, 1);
    mpz_mul_2exp(half, half, 32 * M);
    mpz_sub_ui(half, half, 1);                        // 2^(N'/2) - 1
    int bad = 0, fast = 0, rare = 0, flags = 0, ripple = 0, tdmax = 0;
    auto check = [&](const Val<M> &v, int T, const char *what, int it) {
        // pw_canon
        {
            u64 L[M];
            for (int j = 0; j < M; ++j) L[j] = v.L[j];
            const u32 w0 = (u32)L[0];
            const bool wraps = T > 0 ? (u64)w0 < (u64)T : (u64)w0 + (u64)(-(i64)T) > 0xffffffffull;
            (wraps ? rare : fast)++;
            tovals<M>(want, L, 0);
            mpz_set_si(x, T);
            mpz_sub(want, want, x);                   // L + T 2^N' == L - T
            mpz_mod(want, want, p);
            u64 L2[M];
            for (int j = 0; j < M; ++j) L2[j] = L[j];
            const int fl = pw_canon<M>(L, T);
            // the branch-free form (FAST = false): the same limbs and flag
            const int fl2 = pw_canon<M, false>(L2, T);
            bool same = fl == fl2;
            for (int j = 0; j < M; ++j) same = same && L[j] == L2[j];
            if (!same && bad++ < 5) printf("M=%d canon %s: the two forms differ it=%d T=%d\n", M, what, it, T);
            tovals<M>(got, L, 0);
            bool zero = true;
            for (int j = 0; j < M; ++j) zero = zero && L[j] == 0;
            if (fl) mpz_add(got, got, p), mpz_sub_ui(got, got, 1);   // the flag: 2^N'
            if (mpz_cmp(got, want) || (fl != 0 && fl != 1) || (fl && !zero)) {
                if (bad++ < 5) printf("M=%d canon %s mismatch it=%d T=%d flag=%d\n", M, what, it, T, fl);
            }
            flags += fl;
        }
        // pw_sqrt2
        {
            u64 L[M];
            for (int j = 0; j < M; ++j) L[j] = v.L[j];
            int T2 = T;
            tovals<M>(want, L, T);
            mpz_mul(want, want, half);
            mpz_mod(want, want, p);
            pw_sqrt2<M>(L, T2);
            tovals<M>(got, L, T2);
            mpz_mod(got, got, p);
            const int td = abs(T2) - abs(T);
            if (mpz_cmp(got, want) || td > 3) {
                if (bad++ < 5) printf("M=%d sqrt2 %s mismatch it=%d T=%d -> %d\n", M, what, it, T, T2);
            }
            tdmax = td > tdmax ? td : tdmax;
            // counted: the low half's carry a0 = floor((T - hi - lo) / 2^(N'/2)) met a high half
            // (lo - hi - T) whose low word is below -a0, so the carry ripples
            mpz_import(lo, M / 2, -1, 8, 0, 0, v.L);
            mpz_import(hi, M / 2, -1, 8, 0, 0, v.L + M / 2);
            mpz_set_si(x, T);
            mpz_sub(got, x, hi);
            mpz_sub(got, got, lo);
            mpz_fdiv_q_2exp(got, got, 32 * M);        // a0
            mpz_sub(want, lo, hi);
            mpz_sub(want, want, x);
            mpz_fdiv_r_2exp(want, want, 32);          // the high half's low word
            mpz_neg(got, got);
            ripple += mpz_cmp(want, got) < 0;
        }
    };
    const std::vector<Val<M>> s = placed<M>();
    for (size_t i = 0; i < s.size(); ++i)
        for (int T = -3; T <= 3; ++T) check(s[i], T, "placed", (int)i);
    for (int it = 0; it < 20000; ++it) {
        Val<M> v;
        for (int j = 0; j < M; ++j) v.L[j] = rng();
        if (it % 16 == 1) for (int j = 0; j < M; ++j) v.L[j] &= rng() & rng() & rng();
        if (it % 16 == 2) for (int j = 0; j < M; ++j) v.L[j] |= rng() | rng() | rng();
        if (it % 16 == 3) for (int j = 0; j < M / 2; ++j) v.L[j + M / 2] = v.L[j];   // equal halves
        if (it % 16 == 4) v.L[0] &= ~0xffffffffull;
        if (it % 16 == 5) v.L[0] |= 0xffffffffull;
        check(v, (int)(rng() % 17) - 8, "random", it);
    }
    if (!fast || !rare || !flags || !ripple) {
        printf("M=%d: a case was never reached\n", M);
        ++bad;
    }
    printf("M=%d bad=%d canon: common path %d, wrapped low word %d, 2^N' %d; sqrt2: rippled carry %d, |T'| - |T| <= %d\n", M,
           bad, fast, rare, flags, ripple, tdmax);
    mpz_clears(p, half, x, want, got, lo, hi, NULL);
    return bad;
}

int main()
{
    const int bad = run<10>() + run<18>() + run<20>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
