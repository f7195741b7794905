// Host-side unit test of the precomputed operand's cache record (mpir-fft_amd/csrc/pkernels.hpp):
// the meta word's pack / unpack over every (flag, sign, pending exponent), and pw_mulmod<M> fed an
// operand B that went through a record -- its limbs stored limb-major at [j K + t], its pw_canon
// flag through the meta word, as k_pwsx writes and k_pwsp reads them -- against pw_mulmod on the
// original (Lb, cb) and against GMP, for every inner size the library instantiates (M = 10, 18,
// 20).  The flagged residue 2^N' is covered here: no HBM input makes k_pwsx produce it.
// Stand-alone (own main), so it can also be built with -fsanitize=address,undefined and run directly.
// Built by __graft_entry__.build() (tests/pw_pre_host/Makefile), run by tests/test_pw_pre_host.py.
#include "pkernels.hpp"
#include <gmp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>
static std::mt19937_64 rng(14);
template <int M> void tovals(mpz_t z, const u64 *L, int T) {
    mpz_import(z, M, -1, 8, 0, 0, L);
    mpz_t t; mpz_init_set_si(t, T); mpz_mul_2exp(t, t, 64 * M); mpz_add(z, z, t); mpz_clear(t);
}

// every (flag, sign, P < 2 N') round-trips, and the fields do not overlap
template <int M> int meta_roundtrip() {
    int bad = 0;
    for (int flag = 0; flag < 2; ++flag)
        for (int sign = 0; sign < 2; ++sign)
            for (unsigned P = 0; P < 128u * M; ++P) {
                const u32 w = pw_pre_pack(flag, sign, P);
                int f = -1, s = -1;
                unsigned p = ~0u;
                pw_pre_unpack(w, f, s, p);
                if (f != flag || s != sign || p != P) {
                    if (bad < 5) printf("M=%d meta (%d, %d, %u) -> %08x -> (%d, %d, %u)\n", M, flag, sign, P, w, f, s, p);
                    ++bad;
                }
            }
    return bad;
}

// one slot's record for K threads, thread t's operand in it, as k_pwsx stores and k_pwsp loads
template <int M, int K> struct Record {
    std::vector<unsigned char> bytes;
    Record() : bytes(pw_pre_slot_bytes(M, K), 0xcd) {}
    void store(int t, const u64 (&L)[M], int cb, int S, unsigned P) {
        u64 *rec = (u64 *)bytes.data();
        for (int j = 0; j < M; ++j) rec[j * K + t] = L[j];
        ((u32 *)(rec + M * K))[t] = pw_pre_pack(cb, S, P);
    }
    u32 load(int t, u64 (&L)[M]) const {
        const u64 *rec = (const u64 *)bytes.data();
        for (int j = 0; j < M; ++j) L[j] = rec[j * K + t];
        return ((const u32 *)(rec + M * K))[t];
    }
};

// a (canonical, ca) times b (canonical, cb) with b through the record at thread t
template <int M, int K> int check(Record<M, K> &R, int t, const u64 (&La)[M], int ca, const u64 (&Lb)[M], int cb,
                                  const char *what, mpz_t p) {
    const int S = (int)(rng() & 1);
    const unsigned P = (unsigned)(rng() % (128u * M));
    R.store(t, Lb, cb, S, P);
    u64 Lr[M];
    int fr, sr;
    unsigned pr;
    pw_pre_unpack(R.load(t, Lr), fr, sr, pr);
    int bad = 0;
    if (fr != cb || sr != S || pr != P || memcmp(Lr, Lb, sizeof Lr)) { printf("M=%d %s: the record changed the operand\n", M, what); ++bad; }
    u64 Z[M], Zo[M];
    int T = 99, To = 99;
    pw_mulmod<M>(Z, T, La, ca, Lr, fr);
    pw_mulmod<M>(Zo, To, La, ca, Lb, cb);
    if (T != To || memcmp(Z, Zo, sizeof Z)) { printf("M=%d %s: mulmod on the record differs from mulmod on (Lb, cb)\n", M, what); ++bad; }
    if (T < -1 || T > 0) { printf("M=%d %s: top %d outside {-1, 0}\n", M, what, T); ++bad; }
    mpz_t a, b, want, got; mpz_inits(a, b, want, got, NULL);
    tovals<M>(a, La, ca); tovals<M>(b, Lb, cb);
    mpz_mul(want, a, b); mpz_mod(want, want, p);
    tovals<M>(got, Z, T); mpz_mod(got, got, p);
    if (mpz_cmp(got, want)) { printf("M=%d %s: mulmod on the record differs from GMP\n", M, what); ++bad; }
    mpz_clears(a, b, want, got, NULL);
    return bad;
}

template <int M, int K> int run() {
    mpz_t p; mpz_init(p);
    mpz_set_ui(p, 1); mpz_mul_2exp(p, p, 64 * M); mpz_add_ui(p, p, 1);
    int bad = meta_roundtrip<M>();
    Record<M, K> R;
    // the edge residues as (limbs, flag): 0, 1, 2^N' - 1, the flagged 2^N', 0x80 / 0x7f bytes
    u64 E[6][M];
    int ec[6] = {0, 0, 0, 1, 0, 0};
    const char *en[6] = {"0", "1", "2^N' - 1", "2^N' (flag)", "0x80 bytes", "0x7f bytes"};
    for (int j = 0; j < M; ++j) {
        E[0][j] = 0; E[1][j] = j == 0; E[2][j] = ~0ull; E[3][j] = 0;
        E[4][j] = 0x8080808080808080ull; E[5][j] = 0x7f7f7f7f7f7f7f7full;
    }
    int t = 0;
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k < 6; ++k) {   // every ordered pair, b through the record
            char what[64];
            snprintf(what, sizeof what, "%s x %s", en[i], en[k]);
            bad += check<M, K>(R, t = (t + 37) % K, E[i], ec[i], E[k], ec[k], what, p);
        }
    {   // saturated digits (29-bit: the schoolbook's and M = 18, 20's Karatsuba halves; 30-bit at M = 10)
        for (int DB = 29; DB <= 30; ++DB) {
            const int ND = (64 * M + DB - 1) / DB;
            for (int d = 0; d < ND; ++d) {   // all ones except digit d, and digit d alone
                u64 A[M], B[M];
                for (int j = 0; j < M; ++j) { A[j] = ~0ull; B[j] = 0; }
                for (int b = d * DB; b < (d + 1) * DB && b < 64 * M; ++b) {
                    A[b >> 6] &= ~(1ull << (b & 63));
                    B[b >> 6] |= 1ull << (b & 63);
                }
                bad += check<M, K>(R, t = (t + 37) % K, A, 0, B, 0, "saturated but one digit x one saturated digit", p);
                bad += check<M, K>(R, t = (t + 37) % K, E[2], 0, A, 0, "all digits saturated x saturated but one", p);
                bad += check<M, K>(R, t = (t + 37) % K, B, 0, E[3], 1, "one saturated digit x 2^N'", p);
            }
        }
    }
    for (int it = 0; it < 2000; ++it) {
        u64 A[M], B[M];
        for (int j = 0; j < M; ++j) { A[j] = rng(); B[j] = rng(); }
        if (it % 9 == 4) for (int j = M / 2; j < M; ++j) B[j] = it % 2 ? ~0ull : 0;   // half-empty / half-full
        bad += check<M, K>(R, (int)(rng() % K), A, 0, B, 0, "random", p);
        if (bad > 20) break;
    }
    printf("M=%d record bad=%d\n", M, bad);
    mpz_clear(p);
    return bad;
}

int main()
{
    int bad = run<10, 256>() + run<18, 256>() + run<20, 512>();
    printf(bad ? "FAIL\n" : "OK\n");
    return bad != 0;
}
