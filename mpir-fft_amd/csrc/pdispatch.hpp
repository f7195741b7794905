// pdispatch.hpp -- host-side view of the nested negacyclic pointwise kernel (pkernels.hpp)
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef void (*pw_fn)(uint64_t *, uint64_t *, int *, const uint64_t *, const uint64_t *, const int *, int,
                      uint64_t *, uint64_t *, int *, unsigned long long *);

// k_pwss<M, lk, fuse> (M = inner coefficient limbs, 2^lk pieces; fuse 1: the row DIF's last
// level fused into the load, product to the C arrays; fuse 2: the last two levels, slot quads
// -- their pieces are 4x the inputs', so the plan checks 64 M >= 2 B + lk + 6), nullptr if
// not built
pw_fn pw_get(int M, int lk, int fuse = 0);
size_t pw_lds(int M, int K, int l);

// k_pwsa<M, lk, fuse> (pwsa.hip): the accumulating form, C[slot] <- C[slot] + A[slot] B[slot] at every
// fuse (A and B only read), the same instances, LDS and launch shape as k_pwss; nullptr if not built
typedef void (*pw_acc_fn)(const uint64_t *, const uint64_t *, const int *, const uint64_t *, const uint64_t *, const int *,
                          int, uint64_t *, uint64_t *, int *, unsigned long long *);
pw_acc_fn pw_get_acc(int M, int lk, int fuse = 0);

// k_pwsq<M, lk, fuse>: the squaring form (A <- A^2, no operand B), the same instances, LDS and
// launch shape as k_pwss; nullptr if not built
typedef void (*pw_sq_fn)(uint64_t *, uint64_t *, int *, int, uint64_t *, uint64_t *, int *, unsigned long long *);
pw_sq_fn pw_get_sqr(int M, int lk, int fuse = 0);

// Multiplication by a precomputed operand (pwsp.hip), the same instances, LDS and launch shape:
// k_pwsx<M, lk, fuse>: operand B's slots (through k_pwss's loaders for that fuse) -> the cache, one
// record of pw_pre_record_bytes(M, K) bytes per slot; k_pwsp<M, lk, fuse>: A[slot] times record
// `slot`, to A in place (fuse 0) or to C; nullptr if not built
typedef void (*pw_pre_fn)(const uint64_t *, const uint64_t *, const int *, int, unsigned char *, unsigned long long *);
pw_pre_fn pw_get_pre(int M, int lk, int fuse = 0);
typedef void (*pw_mulpre_fn)(uint64_t *, uint64_t *, int *, const unsigned char *, int, uint64_t *, uint64_t *, int *,
                             unsigned long long *);
pw_mulpre_fn pw_get_mulpre(int M, int lk, int fuse = 0);
size_t pw_pre_record_bytes(int M, int K);

// Small matrix products (pwmm.hip): k_pwmm<M, lk, acc>(caches, stride, kk, ea, eb, l, C): C[slot] (acc: +)=
// the sum of kk <= 4 products of k_pwsx records, record regions ea_i, eb_i (8 bits each) of `stride`
// bytes from `caches`; k_pwss's LDS and launch shape; nullptr if not built
typedef void (*pw_mm_fn)(const unsigned char *, unsigned long long, int, unsigned, unsigned, int, uint64_t *, uint64_t *,
                         int *);
pw_mm_fn pw_get_mm(int M, int lk, bool acc = false);

// Inner ring for a product mod 2^(64 l) + 1 cut into K = 2^lk pieces: the smallest even M
// (limbs) with 64 M >= 2 (64 l / K) + lk + 4: the pair-fused inputs (pieces of x0 +- x1) are
// below 2^(B+1) (1 + 2^-64) in magnitude, so |c_t| < K 2^(2B+2) (1 + 2^-62) < 2^(N'-1)
// and 2 (64 M) a multiple of K (omega = 2^(128 M / K); theta may need sqrt 2: pw_sqrt2).
inline int pw_inner_limbs(long l, int lk)
{
    const long K = 1L << lk, B = 64 * l / K;
    const long need = 2 * B + lk + 4;
    long step = K / 128 > 2 ? K / 128 : 2;   // M even, 128 M multiple of K
    long M = (need + 63) / 64;
    M = (M + step - 1) / step * step;
    return (int)M;
}
