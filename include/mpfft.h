/*
 * mpfft.h -- C ABI of the MI355X-native Schoenhage-Strassen multiplier
 * (libmpfft.so, built from mpir-fft_amd/csrc/ by __graft_entry__.build()).
 *
 * The drop-in entry point is new_mpn_mul, with exactly the reference's
 * signature and meaning:
 *     /root/reference/mul_fft.c:3190-3191
 *     void new_mpn_mul(mp_limb_t *r1, mp_limb_t *i1, mp_size_t n1,
 *                      mp_limb_t *i2, mp_size_t n2,
 *                      mp_bitcnt_t depth, mp_bitcnt_t w);
 * r1[0 .. n1+n2) = i1[0 .. n1) * i2[0 .. n2), little-endian 64-bit limbs,
 * convolution length 2^(depth+1) over Z/(2^(2^depth w) + 1).  The reference
 * checks nothing and "will just segfault" on bad parameters
 * (mul_fft.c:3186-3188); this library validates them and aborts with a message
 * (new_mpn_mul) or returns a status (mpfft_mul_ex / mpfft_mul_device).
 * The result is the exact product, bit-identical to GMP/MPIR mpn_mul and to the
 * reference new_mpn_mul with its pointwise-row fix.
 */
#ifndef MPFFT_H
#define MPFFT_H

#include <stddef.h>
#include <stdint.h>

#if !defined(__GMP_H__) && !defined(__MPIR_H__) && !defined(MPFFT_HAVE_MP_TYPES)
/* GMP/MPIR LP64 types (mp_limb_t 64-bit unsigned, mp_size_t long, mp_bitcnt_t unsigned long) */
typedef uint64_t mp_limb_t;
typedef long mp_size_t;
typedef unsigned long mp_bitcnt_t;
#endif

#define MPFFT_VERSION 10

#define MPFFT_OK 0
#define MPFFT_EINVAL 1          /* n1, n2 < 1; depth outside [2, 30]; n*w not a multiple of 64 */
#define MPFFT_ETOOBIG 2         /* j1 + j2 - 1 > 2^(depth+1): product does not fit */
#define MPFFT_EUNSUPPORTED 3    /* coefficient size n*w/64 > 4096 limbs */
#define MPFFT_ENOMEM 4
#define MPFFT_EHIP 5
#define MPFFT_ENODEV 6

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces new_mpn_mul, mul_fft.c:3190-3265 (host pointers; H2D, device pipeline, D2H). */
void new_mpn_mul(mp_limb_t *r1, mp_limb_t *i1, mp_size_t n1, mp_limb_t *i2, mp_size_t n2,
                 mp_bitcnt_t depth, mp_bitcnt_t w);

/* Same as new_mpn_mul, returning MPFFT_* instead of aborting.  Host pointers.
 * Thread-safe: the calling thread's current HIP device (hipSetDevice) selects a
 * per-device context (stream + grow-only workspace); calls on one device serialise. */
int mpfft_mul_ex(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2,
                 unsigned long depth, unsigned long w);

/* (depth, w) chooser: the reference leaves them to its caller (mul_fft.c:3190-3191).
 * Picks the valid pair (power-of-two w, coefficients of <= 4096 limbs) with the least
 * predicted MI355X time (measured table, profiles/r02/chooser_sweep.json).
 * Returns MPFFT_OK, or MPFFT_ETOOBIG when no supported pair holds the product. */
int mpfft_choose(long n1, long n2, unsigned long *depth, unsigned long *w);

/* mpn_mul-style entry: r1 = i1 * i2 with (depth, w) from mpfft_choose (host pointers). */
int mpfft_mul_auto(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2);

/* Free the calling thread's device context buffers (re-allocated by the next call). */
int mpfft_release(void);

/* Device-resident multiply: all pointers are device memory, work is queued on
 * `stream` (a hipStream_t, NULL = default) and not synchronised.  d_ws must hold
 * mpfft_workspace_bytes(n1, n2, depth, w) bytes.
 * Alignment, for this entry and for the mpfft_sqr_, mpfft_mulmod_, mpfft_mulmodw_, mpfft_mulmodm1_,
 * mpfft_precomp_ / mpfft_mul_precomp_, mpfft_dot_, mpfft_sdot_ and mpfft_matmul_ device and stage entries
 * below: operands and results (d_r, d_i1, d_i2, d_a, d_b and the pointers in a term, entry or result array) need limb
 * (8-byte) alignment only, so rp + k is a valid argument as it is for the mpn_* calls these
 * replace (tests/test_gpu_limb_aligned.py).  mpfft_mul6_device, the mpfft_shard_* entries and
 * mpfft_mul_multi_device read their operands limb by limb as well, but no test runs them on such
 * pointers: give those 16-byte aligned ones.  A workspace d_ws and a cache d_pre must be 256-byte
 * aligned (their arrays sit at 256-byte offsets; hipMalloc returns such pointers); the entries do
 * not check this and return no status for a misaligned one. */
int mpfft_mul_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const uint64_t *d_i2, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);

size_t mpfft_workspace_bytes(long n1, long n2, unsigned long depth, unsigned long w);

/* 0 if (n1, n2, depth, w) is a valid call, else the MPFFT_* reason. */
int mpfft_check_params(long n1, long n2, unsigned long depth, unsigned long w);

/* out[10] = n, l, NC (= sqrt, columns), j1, j2, trunc, bits1, NR (rows), threads/workgroup, limbs/thread
 * (mul_fft.c:3193-3203). */
int mpfft_plan_info(long n1, long n2, unsigned long depth, unsigned long w, long *out);

/* ---- squaring (MPFFT_VERSION 3): r[0 .. 2n) = a[0 .. n)^2, exact, with new_mpn_mul's meaning of
 * (depth, w).  One operand is split and transformed once, the workspace holds no second
 * coefficient array, and the nested pointwise runs its squaring kernel (k_pwsq: one inner forward
 * transform, about half the digit products).  new_mpn_mul / mpfft_mul_ex given the same pointer
 * twice still run the multiply.  Parameter validation and status codes are those of
 * mpfft_check_params(n, n, depth, w); r may not overlap a.
 * Not covered: the sqrt2 front end (new_mpn_mul6), the sharded / multi-GPU entries and
 * mpfft_set_devices routing -- a square always runs on the calling thread's device. */
int mpfft_sqr_ex(uint64_t *r, const uint64_t *a, long n, unsigned long depth, unsigned long w);
/* mpn_sqr-style entry: (depth, w) = mpfft_choose(n, n) (host pointers). */
int mpfft_sqr_auto(uint64_t *r, const uint64_t *a, long n);
/* Device-resident square, queued on `stream`; d_ws holds mpfft_sqr_workspace_bytes(n, depth, w). */
int mpfft_sqr_device(uint64_t *d_r, const uint64_t *d_a, long n, unsigned long depth, unsigned long w,
                     void *d_ws, size_t ws_bytes, void *stream);
/* mpfft_workspace_bytes(n, n, depth, w) less operand B's limb, top and carry-mask arrays. */
size_t mpfft_sqr_workspace_bytes(long n, unsigned long depth, unsigned long w);
/* out[8] as mpfft_workspace_layout, entries 3..5 (the B arrays) 0. */
int mpfft_sqr_workspace_layout(long n, unsigned long depth, unsigned long w, size_t *out);
/* One MPFFT_STAGE_* stage on the square's workspace, operand 0 only. */
int mpfft_sqr_stage(int stage, const uint64_t *d_a, uint64_t *d_r, long n, unsigned long depth,
                    unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* As mpfft_stage_kernels(n, n, ...), the pointwise field "k_pwsq<M>..." on nested plans and
 * "<kernel> (B = A)" where a multiply kernel runs with A's arrays as both operands. */
int mpfft_sqr_stage_kernels(long n, unsigned long depth, unsigned long w, char *buf, size_t len);

/* ---- products mod 2^B + 1 (MPFFT_VERSION 4): r = a b mod M, M = 2^B + 1, B = 64 L, as a
 * length-2n negacyclic convolution mod 2^N + 1 (n = 2^depth, N = n w) of bits1 = B / 2n bit
 * pieces, weighted by the 4n-th root of unity sqrt2^w (the reference's fft_mulmod_2expp1,
 * mul_fft.c:2998-3167): half the slots of the full product at the same coefficient size, and
 * L + 1 limbs over the bus instead of 2 L.
 * Operands and result are L + 1 limbs, fully reduced: 0 <= a <= 2^B, the top limb 0 or 1 and the
 * low L limbs 0 when it is 1 (the host entries return MPFFT_EINVAL otherwise; the device entries
 * do not look).  r may not overlap a or b; d_r may be the next call's operand.
 * Valid (L, depth, w): 2 <= depth <= 30, 64 | N, 2n | 64 L (MPFFT_EINVAL otherwise);
 * 2 bits1 + depth + 2 <= N, so that the signed coefficients can be read back (MPFFT_ETOOBIG);
 * N / 64 <= 4096 (MPFFT_EUNSUPPORTED).  mpfft_mulmod_next_size gives an efficient L.
 * Limits: a negacyclic transform cannot be truncated, so with power-of-two w the fully
 * efficient moduli lie a factor 2 apart (B ~ n^2 w); for B a power of two (Fermat numbers) the
 * pieces are N/4 bits, not N/2, and the slot count equals that of the multiply-and-fold route
 * (the reference's low-limb CRT trick closes that gap: the mpfft_mulmodw_* entries below).
 * Not covered: the sqrt2 front end, the sharded / multi-GPU entries and
 * mpfft_set_devices routing -- these always run on the calling thread's device. */
int mpfft_mulmod_check_params(long L, unsigned long depth, unsigned long w);
int mpfft_mulmod_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w);
/* One operand split, weighted and transformed once; k_pwsq on the nested plans. */
int mpfft_sqrmod_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w);
/* Device-resident, queued on `stream` and not synchronised; d_ws holds
 * mpfft_mulmod_workspace_bytes(L, depth, w, sqr) bytes and need not be cleared. */
int mpfft_mulmod_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                        unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
int mpfft_sqrmod_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                        void *d_ws, size_t ws_bytes, void *stream);
size_t mpfft_mulmod_workspace_bytes(long L, unsigned long depth, unsigned long w, int sqr);
/* out[10] as mpfft_plan_info: j1 = j2 = trunc = 2n, bits1 = 64 L / 2n. */
int mpfft_mulmod_plan_info(long L, unsigned long depth, unsigned long w, long *out);
/* out[8] as mpfft_workspace_layout (sqr: entries 3..5 are 0). */
int mpfft_mulmod_workspace_layout(long L, unsigned long depth, unsigned long w, int sqr, size_t *out);
/* One stage on the mulmod workspace (tests).  MPFFT_STAGE_FWD_COLUMNS: the split + weight launch
 * and the column transform; MPFFT_STAGE_SCALE: the un-weight (slot j by theta^-j 2^-(depth+1),
 * canonical); MPFFT_STAGE_COMBINE: the negacyclic combine of the canonical coefficients into
 * d_r (L + 1 limbs); the others are the multiply's.  MPFFT_STAGE_DRIVEN and
 * MPFFT_STAGE_FOLD_COMBINE return MPFFT_EINVAL. */
int mpfft_mulmod_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                       unsigned long depth, unsigned long w, int sqr, void *d_ws, size_t ws_bytes, void *stream);
/* As mpfft_stage_kernels; the fwd_columns, scale and combine fields name the negacyclic kernels. */
int mpfft_mulmod_stage_kernels(long L, unsigned long depth, unsigned long w, int sqr, char *buf, size_t len);
/* The valid (depth, w) of least predicted time for this L (mpfft_choose's candidates and cost
 * model at 2n slots), MPFFT_ETOOBIG if none is valid. */
int mpfft_mulmod_choose(long L, unsigned long *depth, unsigned long *w);
/* For a caller free to choose the modulus: every candidate's smallest valid L >= min_L (a
 * multiple of its granularity 2n / 64), and of those the (L, depth, w) of least predicted time. */
int mpfft_mulmod_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w);

/* ---- multiplication by a precomputed operand (MPFFT_VERSION 5): for callers that multiply many
 * numbers by the same one (Newton and Barrett steps against a fixed modulus or its inverse, powers
 * of a fixed base, evaluation against a constant).  mpfft_precomp_device runs operand 2's forward
 * stages once -- split, forward columns, forward rows, and on the nested pointwise plans the
 * inner forward transform of every slot (k_pwsx) -- into a cache; mpfft_mul_precomp_device then
 * computes r[0 .. n1 + n2) = i1 * (the cached i2) with operand 1's forward stages alone, the
 * pointwise reading the cache (k_pwsp, or the other pointwise kernels with their B pointers aimed
 * into it), and the multiply's inverse, scaling and combine unchanged: the same exact product.
 * The cache: on nested plans (coefficients of 2048 or 4096 limbs, 1024 under
 * MPFFT_POINTWISE=pwss) one record of K (8 M + 4) bytes per live slot -- 21 504 / 37 888 /
 * 83 968 B at l = 1024 / 2048 / 4096, 2.3-2.6 x the slot itself; elsewhere the live slots of
 * operand 2's transformed coefficient arrays (limbs and carry limbs).  It is bound to
 * (n1, n2, depth, w) -- the truncation depends on both sizes --, to the MPFFT_POINTWISE selection in
 * force when it was made and to the library version (do not store it); it is plain,
 * position-independent device memory, only read by a multiply, so multiplies on different
 * streams with different workspaces may share one cache.
 * Parameter validation and status codes are those of mpfft_check_params(n1, n2, depth, w); a
 * workspace or cache that is too small returns MPFFT_ENOMEM.
 * Not covered: the sqrt2 front end (new_mpn_mul6), the products mod 2^B + 1, the sharded /
 * multi-GPU entries and mpfft_set_devices routing -- these always run on the calling thread's
 * device. */
size_t mpfft_precomp_bytes(long n1, long n2, unsigned long depth, unsigned long w);   /* 0 on invalid parameters */
/* d_i2[0 .. n2) -> d_pre, queued on `stream`; d_ws holds mpfft_workspace_bytes(n1, n2, depth, w). */
int mpfft_precomp_device(void *d_pre, size_t pre_bytes, const uint64_t *d_i2, long n1, long n2,
                         unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* mpfft_workspace_bytes(n1, n2, depth, w) less operand B's limb, top and carry-mask arrays. */
size_t mpfft_mul_precomp_workspace_bytes(long n1, long n2, unsigned long depth, unsigned long w);
/* d_r = d_i1 * cached operand, queued on `stream` and not synchronised; d_ws holds
 * mpfft_mul_precomp_workspace_bytes bytes; d_pre is only read. */
int mpfft_mul_precomp_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const void *d_pre, size_t pre_bytes, long n2,
                             unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* As mpfft_stage_kernels with one extra leading field: what writes the cache ("k_pwsx<M>..." with
 * the pointwise's pair / quad suffix, or "copy"), then the seven stages of a multiply against it,
 * the pointwise "k_pwsp<M>..." on nested plans and "<kernel> (B cached)" elsewhere. */
int mpfft_precomp_stage_kernels(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len);
/* (tests) One stage of the precomputation on the multiply's workspace: MPFFT_STAGE_FWD_COLUMNS and
 * MPFFT_STAGE_FWD_ROWS on operand 2 alone (every row level: none is fused), MPFFT_STAGE_PRE_STORE:
 * operand B's row arrays -> d_pre.  MPFFT_EINVAL on any other stage. */
#define MPFFT_STAGE_PRE_STORE 8
int mpfft_precomp_stage(int stage, void *d_pre, size_t pre_bytes, const uint64_t *d_i2, long n1, long n2,
                        unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* (tests) One MPFFT_STAGE_* stage of the multiply on the workspace without B's arrays, operand 1
 * only; MPFFT_STAGE_POINTWISE reads d_pre. */
int mpfft_mul_precomp_stage(int stage, const uint64_t *d_i1, const void *d_pre, size_t pre_bytes, uint64_t *d_r, long n1,
                            long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* Host pointers: an opaque handle that owns the device cache of i2[0 .. n2) for products with
 * n1-limb operands, bound to the HIP device current at creation.  mpfft_mul_precomp_ex returns
 * MPFFT_EINVAL for another n1, on another device, or after MPFFT_POINTWISE changed the kernel
 * family.  r may not overlap i1. */
typedef struct mpfft_pre mpfft_pre;
int mpfft_precomp_create(mpfft_pre **out, const uint64_t *i2, long n2, long n1, unsigned long depth, unsigned long w);
int mpfft_mul_precomp_ex(uint64_t *r, const uint64_t *i1, long n1, const mpfft_pre *pre);
void mpfft_precomp_destroy(mpfft_pre *pre);

/* ---- products mod 2^B - 1 (MPFFT_VERSION 6): r = a b mod M, M = 2^B - 1, B = 64 L, as a
 * length-2n cyclic convolution mod 2^N + 1 (n = 2^depth, N = n w) of bits1 = B / 2n bit pieces --
 * what the untruncated transform computes as it stands (2^B == 1: GMP's mpn_mulmod_bnm1, the
 * wraparound trick): no weight, no sqrt2, the first column pass splits the operands, and the
 * coefficients are non-negative.  Half the slots of the full product at the same coefficient size
 * and L limbs over the bus instead of 2 L; with the residue mod 2^B + 1 it gives a 2B-bit product
 * by CRT, and where part of a product is already known (Newton and Barrett steps) it recovers the
 * rest.
 * Operands: L limbs each, any value 0 <= a < 2^B (all-ones is accepted; it is 0 mod M).  Result:
 * L limbs, fully reduced, 0 <= r < M -- all-ones is never returned.  r may not overlap a or b;
 * d_r may be the next call's operand.
 * Valid (L, depth, w): 2 <= depth <= 30, 64 | N, 2n | 64 L (MPFFT_EINVAL otherwise);
 * 2 bits1 + depth + 1 <= N, so that c_k <= 2n (2^bits1 - 1)^2 < 2^N (MPFFT_ETOOBIG) -- one bit
 * more room than mod 2^B + 1; N / 64 <= 4096 (MPFFT_EUNSUPPORTED).  mpfft_mulmodm1_next_size gives
 * an efficient L.
 * kind: MPFFT_M1_MUL, MPFFT_M1_SQR (one operand split and transformed once, no B arrays, k_pwsq on
 * the nested plans) or MPFFT_M1_PRE (the multiply against a cached operand: no B arrays either).
 * Limits: the efficient sizes lie a factor 2 apart (B ~ n^2 w with power-of-two w: nothing is
 * truncated); B a power of two has bits1 = N/4.
 * Not covered: the sqrt2 front end, the sharded / multi-GPU entries and mpfft_set_devices
 * routing -- these always run on the calling thread's device. */
#define MPFFT_M1_MUL 0
#define MPFFT_M1_SQR 1
#define MPFFT_M1_PRE 2
int mpfft_mulmodm1_check_params(long L, unsigned long depth, unsigned long w);
/* Host pointers, L limbs each; the operands are not inspected (every value is valid). */
int mpfft_mulmodm1_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w);
int mpfft_sqrmodm1_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w);
/* Device-resident, queued on `stream` and not synchronised; d_ws holds
 * mpfft_mulmodm1_workspace_bytes(L, depth, w, kind) bytes and need not be cleared. */
int mpfft_mulmodm1_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                          unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
int mpfft_sqrmodm1_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                          void *d_ws, size_t ws_bytes, void *stream);
size_t mpfft_mulmodm1_workspace_bytes(long L, unsigned long depth, unsigned long w, int kind);   /* 0 on invalid parameters */
/* out[10] as mpfft_plan_info: j1 = j2 = trunc = 2n, bits1 = 64 L / 2n. */
int mpfft_mulmodm1_plan_info(long L, unsigned long depth, unsigned long w, long *out);
/* out[8] as mpfft_workspace_layout (MPFFT_M1_SQR, MPFFT_M1_PRE: entries 3..5 are 0). */
int mpfft_mulmodm1_workspace_layout(long L, unsigned long depth, unsigned long w, int kind, size_t *out);
/* One stage on the workspace (tests; kind MPFFT_M1_MUL or MPFFT_M1_SQR).  MPFFT_STAGE_FWD_COLUMNS:
 * the split and the column transform; MPFFT_STAGE_SCALE: the plain scaling by 2^-(depth+1),
 * canonical (also where the whole product fuses it into the last inverse column pass);
 * MPFFT_STAGE_COMBINE: the cyclic combine of the canonical coefficients into d_r (L limbs; it
 * clears its own flags); the others are the multiply's.  MPFFT_STAGE_DRIVEN and
 * MPFFT_STAGE_FOLD_COMBINE return MPFFT_EINVAL. */
int mpfft_mulmodm1_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                         unsigned long depth, unsigned long w, int kind, void *d_ws, size_t ws_bytes, void *stream);
/* As mpfft_stage_kernels; the fwd_columns field names the pass that splits, the combine field
 * "k_combine1 + k_cwrap + k_cfix (cyclic)". */
int mpfft_mulmodm1_stage_kernels(long L, unsigned long depth, unsigned long w, int kind, char *buf, size_t len);
/* As mpfft_mulmod_choose / mpfft_mulmod_next_size, for the cyclic bound. */
int mpfft_mulmodm1_choose(long L, unsigned long *depth, unsigned long *w);
int mpfft_mulmodm1_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w);
/* Cached operand (device level; no host handle): mpfft_mulmodm1_precomp_device runs d_b's forward
 * stages once into d_pre (mpfft_mulmodm1_precomp_bytes; d_ws holds the MPFFT_M1_MUL workspace), and
 * mpfft_mulmodm1_mul_precomp_device computes d_r = d_a (the cached b) mod M on the MPFFT_M1_PRE
 * workspace, limb-equal to mpfft_mulmodm1_device.  The cache follows the rules of mpfft_precomp_*:
 * bound to (L, depth, w), to the MPFFT_POINTWISE selection and to the library version, only read
 * by a multiply (streams may share it); a workspace or cache that is too small returns
 * MPFFT_ENOMEM. */
size_t mpfft_mulmodm1_precomp_bytes(long L, unsigned long depth, unsigned long w);   /* 0 on invalid parameters */
int mpfft_mulmodm1_precomp_device(void *d_pre, size_t pre_bytes, const uint64_t *d_b, long L, unsigned long depth,
                                  unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
int mpfft_mulmodm1_mul_precomp_device(uint64_t *d_r, const uint64_t *d_a, const void *d_pre, size_t pre_bytes, long L,
                                      unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);

/* ---- products mod 2^B + 1 with the low-word CRT (MPFFT_VERSION 7): mpfft_mulmod_*'s product with
 * pieces of up to N / 2 + 15 bits, so a power-of-two B (Fermat numbers, Pepin tests, nested
 * Schoenhage-Strassen) runs at bits1 = N / 2: half the transform of mpfft_mulmod_* at the same B.
 * Beside the transform, which gives the coefficients mod p = 2^N + 1, the negacyclic convolution of
 * the pieces' low 32-bit words is computed mod 2^32 (k_nlowconv: 4 n^2 32-bit multiply-adds; the
 * reference's fft_naive_convolution_1 with 32-bit words in place of limbs).  p == 1 (mod 2^32), so
 * the difference of the two, a signed 32-bit word, is floor(c_k / p), and c_k is exact while
 * |c_k| < 2^(N + 31).
 * Operands, result and the rules for r, d_r and the workspace are mpfft_mulmod_*'s.  Valid
 * (L, depth, w): as mpfft_mulmod_check_params with two changes: the bound is
 * 2 bits1 + depth + 2 <= N + 32 (MPFFT_ETOOBIG), and bits1 >= 32 is required (MPFFT_EINVAL): below
 * that the 32-bit words of neighbouring pieces would overlap in the fold, and mpfft_mulmod_* already
 * serves those shapes (2 bits1 + depth + 2 <= 68 <= N + 4 there).  Results are limb-equal to
 * mpfft_mulmod_*'s wherever both are valid.
 * Not covered: the same trick mod 2^B - 1, the cached operand for this family, the sqrt2 front
 * end, the sharded / multi-GPU entries and mpfft_set_devices routing, and fusing the weight or the
 * un-weight into the column passes. */
int mpfft_mulmodw_check_params(long L, unsigned long depth, unsigned long w);
int mpfft_mulmodw_ex(uint64_t *r, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w);
int mpfft_sqrmodw_ex(uint64_t *r, const uint64_t *a, long L, unsigned long depth, unsigned long w);
int mpfft_mulmodw_device(uint64_t *d_r, const uint64_t *d_a, const uint64_t *d_b, long L, unsigned long depth,
                         unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
int mpfft_sqrmodw_device(uint64_t *d_r, const uint64_t *d_a, long L, unsigned long depth, unsigned long w,
                         void *d_ws, size_t ws_bytes, void *stream);
size_t mpfft_mulmodw_workspace_bytes(long L, unsigned long depth, unsigned long w, int sqr);   /* 0 on invalid parameters */
int mpfft_mulmodw_plan_info(long L, unsigned long depth, unsigned long w, long *out);
/* out[9]: the eight entries of mpfft_mulmod_workspace_layout, then the byte offset of the low-word
 * convolution d (2n uint32). */
int mpfft_mulmodw_workspace_layout(long L, unsigned long depth, unsigned long w, int sqr, size_t *out);
/* One stage on the workspace (tests), as mpfft_mulmod_stage, with MPFFT_STAGE_LOWCONV: d from the
 * operands d_a, d_b (sqr: d_a alone); MPFFT_STAGE_COMBINE reads the canonical slots and d from the
 * workspace.  (MPFFT_STAGE_LOWCONV on mpfft_mulmod_stage returns MPFFT_EINVAL.) */
#define MPFFT_STAGE_LOWCONV 9
int mpfft_mulmodw_stage(int stage, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long L,
                        unsigned long depth, unsigned long w, int sqr, void *d_ws, size_t ws_bytes, void *stream);
/* As mpfft_mulmod_stage_kernels; the combine field names k_nlowconv and k_nwrapw.  Under
 * mpfft_profile_begin/end the low-word convolution counts with the combine stage. */
int mpfft_mulmodw_stage_kernels(long L, unsigned long depth, unsigned long w, int sqr, char *buf, size_t len);
/* As mpfft_mulmod_choose / mpfft_mulmod_next_size under this family's bound, the predicted time
 * plus the convolution's 4 n^2 multiply-adds at a measured cost each.  No (depth, w) is valid
 * for L < 4 (bits1 >= 32 at 2n = 8): mpfft_mulmodw_choose returns MPFFT_EINVAL there. */
int mpfft_mulmodw_choose(long L, unsigned long *depth, unsigned long *w);
int mpfft_mulmodw_next_size(long min_L, long *L, unsigned long *depth, unsigned long *w);

/* ---- sums of products (MPFFT_VERSION 8): r[0 .. n1 + n2 + 1) = sum_{i < K} a_i[0 .. n1) b_i[0 .. n2),
 * 1 <= K <= MPFFT_DOT_MAX, exact, single device, with new_mpn_mul's meaning of (depth, w).  Between
 * the forward and the inverse transforms a product is a slot-wise operation on residues mod
 * 2^N + 1, and that stage is linear: every term runs its own forward transforms and pointwise
 * product, the products are added slot-wise in a third coefficient array C, and the inverse
 * transform, the scaling and the combine run once -- for binary splitting (T1 Q2 + P1 T2), the 2x2
 * matrix products of a half-GCD, determinant and resultant steps.
 * The pieces have bits1 = (N - depth - s) / 2 bits, s = ceil(log2 K): a coefficient of the summed
 * convolutions is below K 2^depth (2^bits1 - 1)^2 < 2^N, so it is read off its residue as a single
 * product's is (the multiply's own bits1 leaves no such room when N - depth is even).  The largest
 * operands of a (depth, w) are therefore a few limbs smaller than the multiply's.
 * The result has n1 + n2 + 1 limbs, the top one below K.  Operands are only read; pointers may
 * repeat between terms and a_i == b_i is allowed; r overlaps no operand.
 * Status: MPFFT_EINVAL for K outside [1, MPFFT_DOT_MAX] (and null pointers), MPFFT_ETOOBIG when
 * j1 + j2 - 1 > 2^(depth+1) under that bits1, the rest as mpfft_check_params.  K = 1 is limb-equal
 * to mpfft_mul_device with a zero top limb.
 * Pointwise: the nested family accumulates inside its kernel (k_pwss for the first term, k_pwsa:
 * C <- C + A B for the later ones); the other families form the product in place as the multiply
 * does and add it with k_slotacc.  The workspace holds three coefficient arrays whatever K.
 * Under mpfft_profile_begin/end every term claims a call slot (max_calls >= K per sum): the
 * forward and pointwise stage times are sums over the terms, the returned call count counts terms.
 * Signed terms (a b - c d) are the mpfft_sdot_* entries below.
 * Matrix products with shared forward transforms and one inner inverse per result entry are the
 * mpfft_matmul_* entries below.
 * Not covered: squares as terms (a_i == b_i runs as a product), the
 * sqrt2 front end, the mod 2^B +- 1 families, the sharded / multi-GPU entries and
 * mpfft_set_devices routing. */
#define MPFFT_DOT_MAX 64
int mpfft_dot_check_params(long K, long n1, long n2, unsigned long depth, unsigned long w);
/* out[10] as mpfft_plan_info */
int mpfft_dot_plan_info(long K, long n1, long n2, unsigned long depth, unsigned long w, long *out);
/* mpfft_choose's candidates and cost model under the dot bound */
int mpfft_dot_choose(long K, long n1, long n2, unsigned long *depth, unsigned long *w);
size_t mpfft_dot_workspace_bytes(long K, long n1, long n2, unsigned long depth, unsigned long w);   /* 0 on invalid parameters */
/* out[11]: the eight entries of mpfft_workspace_layout, then the byte offsets of C's limb, top and
 * carry-mask arrays. */
int mpfft_dot_workspace_layout(long K, long n1, long n2, unsigned long depth, unsigned long w, size_t *out);
/* d_a, d_b: host arrays of K device pointers (read during the call only).  Queued on `stream`, not
 * synchronised. */
int mpfft_dot_device(uint64_t *d_r, long K, const uint64_t *const *d_a, const uint64_t *const *d_b, long n1, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* Host pointers: a, b arrays of K host operands; they go through the device context's buffers term
 * by term.  mpfft_dot_auto: (depth, w) from mpfft_dot_choose. */
int mpfft_dot_ex(uint64_t *r, long K, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2,
                 unsigned long depth, unsigned long w);
int mpfft_dot_auto(uint64_t *r, long K, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2);
/* As mpfft_stage_kernels; the pointwise field names the first term's kernel and the later terms':
 * "k_pwss<M>... + k_pwsa<M>..." (with the pair / quad suffix) on nested plans, "<kernel> + k_slotacc"
 * elsewhere. */
int mpfft_dot_stage_kernels(long K, long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len);
/* (tests) One MPFFT_STAGE_* stage for one term (d_a, d_b single operands) on the dot plan and
 * workspace.  MPFFT_STAGE_POINTWISE writes C <- A B (A's arrays are overwritten); or-ed with
 * MPFFT_STAGE_ACC it computes C <- C + A B (the nested family reads A and B only, the others
 * overwrite A).  The stages behind the pointwise read C.  Like mpfft_stage it never fuses row
 * levels.  MPFFT_STAGE_ACC on any other stage returns MPFFT_EINVAL. */
#define MPFFT_STAGE_ACC 0x200
int mpfft_dot_stage(int stage, long K, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1, long n2,
                    unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);

/* ---- signed sums of products (MPFFT_VERSION 9): r[0 .. n1 + n2 + 1) = sum_{i < K} s_i a_i b_i, s_i = -1
 * where bit i of `neg` is set and +1 elsewhere -- determinants (a d - b c), a half-GCD matrix applied
 * to a vector, CRT recombinations, resultant steps, Newton residuals (1 - x d) -- on the plan, the
 * (depth, w) validity, the operand bound and the chooser of mpfft_dot_* (use mpfft_dot_choose and
 * mpfft_dot_plan_info), with K forward transform pairs and one inverse.
 * Exact, no bit of headroom lost: with X = 2^(64 n1), a term that is subtracted feeds the transforms
 * the limb-wise complement ~a_i = X - 1 - a_i (n1 limbs, non-negative, the same number of pieces), so
 * the unsigned sum comes out as r' = r + (X - 1) D, D = sum_neg b_i (at most n2 + 1 limbs), and
 * r = r' - X D + D mod 2^(64 (n1 + n2 + 1)).  Every piece stays in [0, 2^bits1) and every coefficient
 * below 2^N under the dot plan's bits1; the transform, pointwise, accumulate, inverse and combine
 * kernels run as they do for mpfft_dot_*.  Two streaming steps are added: per negative term k_sdneg
 * (~a_i into a scratch the split reads, D <- D + b_i in carry-save form, the first negative term
 * initialising D) and, once behind the combine, d_r <- d_r + D - (D << 64 n1) in place (k_sdedge +
 * k_sdfix: the reduced-form combine's signed carry chain over blocks of MPFFT_SDOT_FIX_BLOCK limbs).
 * A fixed number of launches per sum, no host synchronisation; neg == 0 launches neither and is
 * limb-equal to mpfft_dot_*.
 * Result: n1 + n2 + 1 limbs, the two's-complement value of the signed sum (|r| < 64 2^(64 (n1 + n2)));
 * the sign is bit 63 of the top limb, which lies in [0, K) or [2^64 - K, 2^64).  Operands are only
 * read; pointers may repeat between terms, whatever their signs, and a_i == b_i is allowed; r
 * overlaps no operand.
 * Status: MPFFT_EINVAL if `neg` has a bit at or above K, everything else as mpfft_dot_check_params; a
 * workspace that is too small returns MPFFT_ENOMEM.
 * Workspace: the dot workspace followed by the complement scratch (8 n1 bytes) and D, every offset
 * 256-byte aligned; its size does not depend on `neg`, it need not be cleared, and a dot workspace laid
 * at its front is valid for mpfft_dot_stage.
 * Under mpfft_profile_begin/end the pre-pass counts with its term's forward-columns stage and the
 * correction with the combine stage; call slots stay one per term.
 * Not covered: the complement fused into the split loads (it would save the scratch's round trip,
 * 16 n1 bytes per negative term), the correction fused into the combine (16 (n1 + n2 + 1) bytes per
 * sum), signed terms on the mod 2^B +- 1 families, the sqrt2 front end, the sharded / multi-GPU
 * entries and mpfft_set_devices routing, shared forward transforms between terms. */
#define MPFFT_SDOT_FIX_BLOCK 4096   /* limbs per block of the correction's carry chain */
int mpfft_sdot_check_params(long K, uint64_t neg, long n1, long n2, unsigned long depth, unsigned long w);
size_t mpfft_sdot_workspace_bytes(long K, long n1, long n2, unsigned long depth, unsigned long w);   /* 0 on invalid parameters */
/* out[13]: the eleven entries of mpfft_dot_workspace_layout, then the byte offsets of the complement
 * scratch (n1 limbs) and of D (n2 limbs, behind them one overflow byte per limb). */
int mpfft_sdot_workspace_layout(long K, long n1, long n2, unsigned long depth, unsigned long w, size_t *out);
/* As mpfft_dot_device; d_ws holds mpfft_sdot_workspace_bytes bytes. */
int mpfft_sdot_device(uint64_t *d_r, long K, uint64_t neg, const uint64_t *const *d_a, const uint64_t *const *d_b,
                      long n1, long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* Host pointers, term by term through the device context's buffers as mpfft_dot_ex (D lives on the
 * device: no operand is kept after its term).  mpfft_sdot_auto: (depth, w) from mpfft_dot_choose. */
int mpfft_sdot_ex(uint64_t *r, long K, uint64_t neg, const uint64_t *const *a, const uint64_t *const *b,
                  long n1, long n2, unsigned long depth, unsigned long w);
int mpfft_sdot_auto(uint64_t *r, long K, uint64_t neg, const uint64_t *const *a, const uint64_t *const *b, long n1, long n2);
/* mpfft_dot_stage_kernels' seven fields; when neg != 0 the fwd_columns field is prefixed by
 * "k_sdneg + " and the combine field suffixed by " + k_sdedge + k_sdfix (blocks of 4096 limbs)". */
int mpfft_sdot_stage_kernels(long K, uint64_t neg, long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len);
/* (tests) The two stages of this family on its workspace; every other stage is forwarded to
 * mpfft_dot_stage on the same workspace.  MPFFT_STAGE_ACC on anything but MPFFT_STAGE_POINTWISE and
 * MPFFT_STAGE_SD_NEG returns MPFFT_EINVAL. */
#define MPFFT_STAGE_SD_NEG 10   /* d_a -> complement scratch, D <- d_b; or-ed with MPFFT_STAGE_ACC: D <- D + d_b */
#define MPFFT_STAGE_SD_FIX 11   /* d_r <- d_r + D - (D << 64 n1), n1 + n2 + 1 limbs */
int mpfft_sdot_stage(int stage, long K, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1, long n2,
                     unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);

/* ---- small matrix products (MPFFT_VERSION 10): R = X Y, R[i][j] = sum_{t < k} X[i][t] Y[t][j], X m x k with
 * entries of n1 limbs, Y k x p with entries of n2 limbs, R m x p with entries of n1 + n2 + 1 limbs (the top
 * one below k), 1 <= m, k, p <= MPFFT_MM_MAX, exact, single device, with new_mpn_mul's meaning of
 * (depth, w) -- the 2x2 by 2x2 and 2x2 by 2x1 products of binary splitting, half-GCD steps and
 * determinants, which as m p calls of mpfft_dot_device transform every operand p (or m) times.
 * Plan, (depth, w) validity, operand bound and chooser are mpfft_dot_*'s at K = k: use
 * mpfft_dot_choose(k, n1, n2), mpfft_dot_plan_info and the bindings' dot_max_limbs.  Every R[i][j] is
 * limb-equal to mpfft_dot_device on the same k terms; (1, k, 1) is the dot, (1, 1, 1) the multiply with a
 * zero top limb.  Operands are only read; pointers may repeat anywhere in X and Y, X[i][t] == Y[t][j]
 * included when n1 == n2; no result overlaps an operand or another result.  Matrices are row-major arrays
 * of pointers.
 * Forward side, once per matrix entry (m k + k p single-operand forward transforms): split, forward
 * columns and rows, then the entry's transformed slots go to a cache region in the workspace, in
 * mpfft_precomp_*'s layout -- on nested plans k_pwsx records, the slots after the inner forward transform,
 * the row levels the plan fuses paid there once.  Per result entry: on nested plans k_pwmm multiplies the
 * k pairs of records of a slot, adds the products with their signs in the inner ring (the pending
 * exponents of a record depend on the thread alone, so no product is rotated) and runs one inner
 * inverse and one output stage; the other families copy X's cached slots into a staging array, run the
 * multiply's pointwise in place with B read from Y's cache and add with k_slotacc (a correctness path,
 * not tuned).  The multiply's inverse rows, truncated inverse columns, scaling and combine then run once
 * per result entry, each combine clearing its own look-back flags and ticket counter.  A fixed number
 * of launches per product, no host synchronisation.
 * Status: MPFFT_EINVAL for m, k or p outside [1, MPFFT_MM_MAX] (and null pointers), MPFFT_ENOMEM for a
 * workspace that is too small, the rest as mpfft_dot_check_params(k, ...).
 * Workspace: the dot workspace at K = k (A's and B's arrays stage an X and a Y operand's forward
 * transform, C holds one result entry's sum), then m k + k p cache regions at a uniform stride, X's
 * entries row-major first; every offset 256-byte aligned.  Its size depends on the shape alone, it need
 * not be cleared, and a dot workspace laid at its front is valid for mpfft_dot_stage.
 * Under mpfft_profile_begin/end a product claims m k + k p + m p call slots: one per matrix entry, whose
 * forward-columns and forward-rows stages are that operand's and whose pointwise stage is its cache
 * store (the later stages empty), then one per result entry, whose forward stages are empty, whose
 * pointwise stage is the sum over its k terms and whose later stages are its inverse side.  The stage
 * times returned are the product's, the call count m k + k p + m p.
 * Not covered: signed entries, a persistent matrix handle applied to many vectors (the caches live in
 * the workspace and are rewritten by every call), squares as terms, the mod 2^B +- 1 families, the sqrt2
 * front end, the sharded / multi-GPU entries and mpfft_set_devices routing. */
#define MPFFT_MM_MAX 4
int mpfft_matmul_check_params(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w);
size_t mpfft_matmul_workspace_bytes(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w);   /* 0 on invalid parameters */
/* out[14]: the eleven entries of mpfft_dot_workspace_layout(k, ...), then the byte offset of cache 0, the
 * stride between caches in bytes and their number m k + k p (X[i][t] is cache i k + t, Y[t][j] cache
 * m k + t p + j). */
int mpfft_matmul_workspace_layout(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w, size_t *out);
/* d_r: host array of m p device pointers, d_a of m k, d_b of k p, row-major (read during the call only).
 * Queued on `stream`, not synchronised. */
int mpfft_matmul_device(uint64_t *const *d_r, long m, long k, long p, const uint64_t *const *d_a, const uint64_t *const *d_b,
                        long n1, long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
/* Host pointers: the operands go through the device context's io buffer one at a time.
 * mpfft_matmul_auto: (depth, w) from mpfft_dot_choose(k, n1, n2). */
int mpfft_matmul_ex(uint64_t *const *r, long m, long k, long p, const uint64_t *const *a, const uint64_t *const *b, long n1,
                    long n2, unsigned long depth, unsigned long w);
int mpfft_matmul_auto(uint64_t *const *r, long m, long k, long p, const uint64_t *const *a, const uint64_t *const *b, long n1,
                      long n2);
/* mpfft_dot_stage_kernels' seven fields; the pointwise field reads "k_pwsx<M>... + k_pwmm<M> (single launch,
 * K=...)" on nested plans (one launch for a result entry's k terms: it measured faster than k launches of one
 * term each at every M), "<kernel> (B cached) + k_slotacc" elsewhere. */
int mpfft_matmul_stage_kernels(long m, long k, long p, long n1, long n2, unsigned long depth, unsigned long w, char *buf,
                               size_t len);
/* (tests) The two stages of this family on its workspace; every other stage is forwarded to
 * mpfft_dot_stage(stage, k, ...) on the dot workspace at the front (kk, ea, eb unused).  Like
 * mpfft_dot_stage it never fuses row levels.  MPFFT_STAGE_MM_STORE: the row arrays of operand 0 (A's
 * arrays, for a cache of X: ea[0] < m k) or operand 1 (B's) -> cache ea[0].  MPFFT_STAGE_MM_POINTWISE:
 * C <- sum_{i < kk} cache ea[i] * cache eb[i] over the live slots, 1 <= kk <= MPFFT_MM_MAX, any cache
 * indices; or-ed with MPFFT_STAGE_ACC: C <- C + that sum.  On the families that multiply in place A's
 * arrays are overwritten. */
#define MPFFT_STAGE_MM_STORE 12
#define MPFFT_STAGE_MM_POINTWISE 13
int mpfft_matmul_stage(int stage, long m, long k, long p, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_r, long n1,
                       long n2, unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream, long kk,
                       const int *ea, const int *eb);

/* ---- sqrt2 front end: replaces new_mpn_mul6, mul_fft.c:3573-3668 ----------------------
 * A length-4n convolution mod 2^N + 1 (N = 2^depth w) through the 4n-th root of unity
 * sqrt2^w, sqrt2 = 2^(3N/4) - 2^(N/4): twice the transform length of new_mpn_mul at the
 * same coefficient size, bits1 = (N - depth - 1)/2 (:3578).  Any w with 64 | N (odd w is
 * where sqrt2 matters).  The reference needs trunc > 2n; here smaller products also work. */
void new_mpn_mul6(mp_limb_t *r1, mp_limb_t *i1, mp_size_t n1, mp_limb_t *i2, mp_size_t n2,
                  mp_bitcnt_t depth, mp_bitcnt_t w);
int mpfft_mul6_ex(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2,
                  unsigned long depth, unsigned long w);
int mpfft_mul6_device(uint64_t *d_r, const uint64_t *d_i1, long n1, const uint64_t *d_i2, long n2,
                      unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);
size_t mpfft_workspace_bytes6(long n1, long n2, unsigned long depth, unsigned long w);
int mpfft_check_params6(long n1, long n2, unsigned long depth, unsigned long w);
/* out[10] as mpfft_plan_info, for new_mpn_mul6 (mul_fft.c:3575-3603) */
int mpfft_plan_info6(long n1, long n2, unsigned long depth, unsigned long w, long *out);

/* Byte offsets inside a single-GPU workspace (tests / multi-GPU driver):
 * out[8] = digA, topA, cbA, digB, topB, cbB, slots per operand, carry-mask words per slot. */
int mpfft_workspace_layout(long n1, long n2, unsigned long depth, unsigned long w, size_t *out);

/* One stage of the pipeline on a single-GPU workspace (stage-parity tests, multi-GPU driver). */
#define MPFFT_STAGE_FWD_COLUMNS 0   /* split + truncated column DIF, both operands   (mul_fft.c:2374-2390) */
#define MPFFT_STAGE_FWD_ROWS 1      /* MFA twiddle + row DIF, canonical out           (mul_fft.c:2392-2408) */
#define MPFFT_STAGE_POINTWISE 2     /* mpn_mulmod_2expp1 over the trunc live slots    (mul_fft.c:3244-3253) */
#define MPFFT_STAGE_INV_ROWS 3      /* row DIT + MFA un-twiddle                       (mul_fft.c:2942-2957) */
#define MPFFT_STAGE_INV_COLUMNS 4   /* truncated column inverse                       (mul_fft.c:2959-2977) */
#define MPFFT_STAGE_SCALE 5         /* divide by 2^(depth+1), normalise               (mul_fft.c:3256-3260) */
#define MPFFT_STAGE_COMBINE 6       /* FFT_combine_bits                               (mul_fft.c:3261-3262) */
#define MPFFT_NSTAGES 7
/* (tests) the folded path's combine: the workspace's coefficients as the inverse
 * columns leave them -- reduced form, 2^-(depth+1) already applied, the rows the truncated
 * inverse doubles not yet doubled -- into the product; MPFFT_EUNSUPPORTED on plans that do not
 * fold (mpfft_stage_kernels names k_combine_red for them) */
#define MPFFT_STAGE_FOLD_COMBINE 7
/* (tests) or-ed onto MPFFT_STAGE_INV_ROWS, _INV_COLUMNS or _SCALE: the stage runs as the whole
 * multiply drives it (Exec::drive_single) instead of in the stand-alone stage mode -- on fold plans
 * 2^-(depth+1) rides in the last inverse row pass, or with the inverse MFA twiddle in the first
 * pass of each column block; the truncated inverse leaves its top-level doubling of rows
 * [dbl_lo, dbl_hi) undone, and SCALE (a no-op on fold plans) applies it.  After driven INV_ROWS and
 * INV_COLUMNS a fold plan's slots are what MPFFT_STAGE_FOLD_COMBINE reads; on the other plans
 * driven INV_ROWS, INV_COLUMNS, SCALE leave the canonical coefficients.  MPFFT_EINVAL on any other
 * stage. */
#define MPFFT_STAGE_DRIVEN 0x100
int mpfft_stage(int stage, const uint64_t *d_i1, const uint64_t *d_i2, uint64_t *d_r, long n1, long n2,
                unsigned long depth, unsigned long w, void *d_ws, size_t ws_bytes, void *stream);

/* ---- multi-GPU: one rank's share of a column-sharded multiply (mpir-fft_amd/sharded.py) ----
 * Column layout (column passes, ITFT, scale): slot = pos * ccount + (c - c0), NR * ccount slots.
 * Row layout (row passes, pointwise, combine): rows r0 .. r0+rcount of NC/ccb column blocks,
 *   slot = (c / ccb) * rcount * ccb + (p - r0) * ccb + c % ccb, rcount * NC slots.
 * Each slot: dig[l] limbs, cb[cb_words] carry masks, top int32. */
typedef struct mpfft_shard {
    long n1, n2;
    unsigned long depth, w;
    int c0, ccount;           /* columns of the column passes */
    int r0, rcount;           /* computed row positions of the row passes */
    int ccb;                  /* columns per block of the row layout (= NC / ranks) */
    uint64_t *col_dig[2], *col_cb[2];
    int *col_top[2];
    uint64_t *row_dig[2], *row_cb[2];
    int *row_top[2];
    long src_chunk;           /* 0: d_i1/d_i2 are the whole operands; else this rank's column
                                 slices: for each position p < T/NC, `src_chunk` limbs from
                                 limb floor((p NC + c0) bits1 / 64) on (sharded.py) */
    /* optional third row-layout array (NULL: none).  When set and mpfft_shard_row_fused()
     * says so, the row DIF's last level runs inside the pointwise, whose product lands here
     * (the caller then treats it as the row array of operand 0).  Added in MPFFT_VERSION 2:
     * callers must zero-initialise the whole struct (memset or `= {0}`), so code written for
     * the version-1 layout that sets only the older fields passes NULL here; a non-NULL
     * triple is always taken as a live array. */
    uint64_t *rowc_dig, *rowc_cb;
    int *rowc_top;
} mpfft_shard;

/* 1 if the sharded row stages fuse the last row DIF level into the pointwise for these
 * parameters and ccb columns per row block (the caller then supplies rowc_*), else 0. */
int mpfft_shard_row_fused(long n1, long n2, unsigned long depth, unsigned long w, int ccb);

#define MPFFT_SHARD_FWD_COLUMNS 0   /* split + column DIF of both operands (column layout) */
#define MPFFT_SHARD_FWD_ROWS 1      /* twiddle + row DIF of both operands (row layout), canonical */
#define MPFFT_SHARD_POINTWISE 2     /* row layout A <- A * B */
#define MPFFT_SHARD_INV_ROWS 3      /* row DIT + un-twiddle of A (row layout) */
#define MPFFT_SHARD_INV_COLUMNS 4   /* truncated column inverse + scale of A (column layout), canonical */
#define MPFFT_SHARD_FWD_COLUMNS_A 5 /* MPFFT_SHARD_FWD_COLUMNS for operand 1 only (clears the combine flags) */
#define MPFFT_SHARD_FWD_COLUMNS_B 6 /* ... for operand 2 only: with _A, lets operand 1's exchange overlap it */
#define MPFFT_SHARD_FWD_COLUMNS_OWN 7 /* MPFFT_SHARD_FWD_COLUMNS, but only rows [r0, r0 + rcount) of the
                                         column layout are computed (replicated forward columns: every
                                         rank runs every column block for its own rows) */
int mpfft_shard_stage(int stage, const mpfft_shard *sh, const uint64_t *d_i1, const uint64_t *d_i2, void *stream);
/* The row stages (FWD_ROWS, POINTWISE, INV_ROWS) on local rows [lo, hi) of the shard only, so a
 * driver can run the row phase in chunks and start exchange #2 of a finished chunk early. */
int mpfft_shard_stage_rows(int stage, const mpfft_shard *sh, int lo, int hi, void *stream);

/* Combine the canonical coefficients of a rank's column layout (after MPFFT_SHARD_INV_COLUMNS)
 * into its product stripes.  The product is cut into S = world * Tr stripes
 * (mpfft_shard_partition): stripe s owns coefficients [s C, (s+1) C) and product limbs
 * [ms[s], ms[s+1]) (mpfft_shard_stripes).  Rank g (= c0 / ccount) holds stripes s = j world + g,
 * j < Tr -- its column-layout rows -- and writes stripe j's limbs to d_r + j SL.
 * d_halo: the H coefficients before each of its stripes (l limbs each; stripe j's at
 * d_halo + j H l), moved there by the copies of mpfft_shard_halo_plan.
 * phase 0: every stripe with carry-in 0; d_sums[2 j], [2 j + 1] = (carry out, every limb
 *          all-ones) of stripe j.
 * phase 1: d_sums_all = the world ranks' d_sums in rank order (world * Tr * 2 ints, e.g. an
 *          all-gather): adds the carry from the stripes below to each of the rank's stripes.
 * Both phases are queued on `stream`; nothing synchronises with the host. */
size_t mpfft_shard_combine_tmp_bytes(long n1, long n2, unsigned long depth, unsigned long w, int world);
int mpfft_shard_combine(const mpfft_shard *sh, int phase, uint64_t *d_r, const uint64_t *d_halo, int *d_sums,
                        const int *d_sums_all, void *d_tmp, size_t tmp_bytes, void *stream);

/* ---- multi-GPU from one C process (north_star: "host code stays C") ----------
 * The same column-sharded multiply as mpir-fft_amd/sharded.py (one process per GPU over
 * RCCL), driven from one host thread over G devices: every rank's stages on its own device
 * stream, the two exchanges and the halo as peer copies over xGMI (hipMemcpyPeerAsync; peer
 * access enabled between distinct devices), ordered by events; the stripe carries on the device.
 * (Tested with every rank on one device; the cross-device copies have not run on separate GPUs.)
 *
 * Partition of one multiply over `world` ranks (a power of two dividing the plan's NC,
 * out[2] of mpfft_plan_info -- at l = 2048 in truncation case b that is 2^(floor(depth/2)+1),
 * not the reference's 2^floor(depth/2)):
 *   rows[world + 1]  row positions: rank d owns live rows [rows[d], rows[d+1])
 *   info[7]          C (columns per rank), chunk (operand slice limbs per row position),
 *                    H (halo coefficients per stripe), Tr (= trunc / NC), fused (1: the
 *                    pointwise takes the row DIF's last level(s), mpfft_shard_row_fused at
 *                    ccb = C), SL (product limbs per stripe at most: the d_r stride),
 *                    S (stripes = world Tr) */
int mpfft_shard_partition(long n1, long n2, unsigned long depth, unsigned long w, int world,
                          long *rows, long *info);
/* ms[0 .. S] = the first product limb of each stripe (ms[S] = n1 + n2); returns S + 1, or
 * -MPFFT_* (cap: ms's capacity; ms == NULL: counted only). */
long mpfft_shard_stripes(long n1, long n2, unsigned long depth, unsigned long w, int world, long *ms, long cap);

/* One exchange as element copies between the ranks' arrays (column layout: NR*C slots per
 * operand; row layout: (rows[d+1]-rows[d])*NC slots), fields dig (l u64 per slot), cb
 * (cb_words u64 per slot), top (one int32 per slot). */
typedef struct mpfft_copy {
    int src, dst;              /* ranks */
    int op;                    /* operand 0 or 1 */
    int field;                 /* 0 dig, 1 cb, 2 top */
    int src_layout, dst_layout;    /* 0 column layout, 1 row layout */
    long src_off, dst_off, count;  /* in elements of the field */
} mpfft_copy;
#define MPFFT_XCHG_COL_TO_ROW 1   /* #1 after the forward columns: both operands, every field */
#define MPFFT_XCHG_ROW_TO_COL 2   /* #2 after the inverse rows: operand 0, every field */
#define MPFFT_LAYOUT_HALO 2       /* mpfft_copy.dst_layout of a halo copy: the receiver's d_halo */
/* Number of copies written to out (out == NULL: counted only; cap: out's capacity),
 * or -MPFFT_* on error. */
long mpfft_shard_exchange_plan(long n1, long n2, unsigned long depth, unsigned long w, int world, int which,
                               mpfft_copy *out, long cap);
/* The halo copies before the combine: for every stripe, the H coefficients before it, from
 * the column layout (canonical limbs, field 0) of the ranks holding them to the d_halo of
 * mpfft_shard_combine (dst_layout MPFFT_LAYOUT_HALO); offsets and counts in limbs.  At most a
 * few coefficients per stripe: this replaces moving the whole product to row owners. */
long mpfft_shard_halo_plan(long n1, long n2, unsigned long depth, unsigned long w, int world,
                           mpfft_copy *out, long cap);

/* r1 = i1 * i2 (host pointers) sharded over ngpus devices: devices[g] is rank g's HIP device
 * (NULL: 0 .. ngpus-1; a device may repeat -- ranks sharing one GPU, as the tests do).
 * ngpus must be a power of two dividing the plan's NC (mpfft_shard_partition).  Device
 * buffers are cached per device list (grow-only; mpfft_multi_release frees them).  Not
 * reentrant with itself: concurrent calls serialise on one lock. */
int mpfft_mul_multi(uint64_t *r1, const uint64_t *i1, long n1, const uint64_t *i2, long n2,
                    unsigned long depth, unsigned long w, int ngpus, const int *devices);

/* The operand slices rank `rank` of `world` reads (the device-resident entry's inputs):
 * mpfft_shard_src_limbs limbs per operand -- for each live row position q, `chunk` limbs from
 * limb floor((q NC + c0) bits1 / 64) on, of the rank's own column block, or of every block
 * in turn when the forward columns are replicated (two ranks; MPFFT_REPLICATE_COLUMNS). */
long mpfft_shard_src_limbs(long n1, long n2, unsigned long depth, unsigned long w, int world);
int mpfft_shard_pack(long n1, long n2, unsigned long depth, unsigned long w, int world, int rank,
                     const uint64_t *a, long na, uint64_t *out);

/* Device-resident multi-GPU multiply: d_src1[g], d_src2[g] are rank g's packed operand slices
 * (mpfft_shard_pack) in devices[g]'s memory; rank g's product stripes land in d_r[g]
 * (stripe j -- product limbs [ms[j world + g], ms[j world + g + 1]) -- at d_r[g] + j SL, Tr SL
 * limbs).  streams[g] (hipStream_t on devices[g]): the work starts after what is queued there
 * and is queued back onto it (nothing waits on the host); streams == NULL: the call returns
 * when the product is complete. */
int mpfft_mul_multi_device(long n1, long n2, unsigned long depth, unsigned long w, int ngpus, const int *devices,
                           const uint64_t *const *d_src1, const uint64_t *const *d_src2, uint64_t *const *d_r,
                           void *const *streams);
int mpfft_multi_release(void);
/* The event graph of `calls` back-to-back mpfft_mul_multi_device calls over `world` ranks, as
 * text (no GPU touched, nothing allocated): one line per cross-stream ordering and per queued
 * piece of work -- "R d S ev" record, "W d S e ev" wait, "K d S what" rank-local work,
 * "C d S what e" a copy from rank e, "N" next call (multi.hip, the event graph).  Returns the
 * bytes needed including the terminating 0 (buf may be null), or a negative MPFFT_E* code. */
long mpfft_multi_schedule(long n1, long n2, unsigned long depth, unsigned long w, int world, int calls, char *buf,
                          size_t len);

/* new_mpn_mul / mpfft_mul_ex policy: with ngpus > 1 devices set, products whose coefficients
 * have >= min_l limbs (0: 1024) and whose NC the device count divides run through
 * mpfft_mul_multi; everything else on the calling thread's device as before.  ngpus <= 1
 * turns it off.  The environment variable MPFFT_DEVICES="0,1,...,7" (read at the first
 * multiply) sets the same policy for callers that cannot call this (an unmodified MPIR). */
int mpfft_set_devices(int ngpus, const int *devices, long min_l);
/* Devices the calling thread's last mpfft_mul_ex / new_mpn_mul ran on (1: single device). */
int mpfft_last_ngpus(void);

/* Stage profiling of the whole-multiply entries (new_mpn_mul, mpfft_mul_ex,
 * mpfft_mul_device, the squares mpfft_sqr_ex / mpfft_sqr_device, the multiplies against a precomputed
 * operand and the precomputation itself -- its last stage is the store into the cache, the four
 * after it read 0 --, and the products mod 2^B + 1, where
 * the weight launch counts with the forward columns, the un-weight is the scale stage and the
 * negacyclic combine the combine stage): between begin and end, each of the next max_calls multiplies
 * records a HIP event on its own stream at every stage boundary (no other change to
 * the work); end synchronises and returns the summed per-stage milliseconds
 * (stage_ms[MPFFT_NSTAGES], MPFFT_STAGE_* order) and the number of profiled calls. */
int mpfft_profile_begin(int max_calls);
/* The kernel that carries each stage for these parameters, ';'-separated in MPFFT_STAGE_* order.
 * Where k_rpass also splits the operands, the forward-column entry names that first pass's
 * instance: "k_rpass (split: k_rpass<LOGG,PP,0,2>)". */
int mpfft_stage_kernels(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len);
/* The launches of the single-device truncated inverse column transform for these parameters, one
 * per line, in order (a host-side dry run; no device needed): "k_rpass<levels,l/1024,dir,mode> pos
 * off+len [fill lo= off=] [halfadd d1..d0]", "k_rpair<l/1024,op> off= h= i0= cnt=", "k_rchain<..>".
 * MPFFT_EINVAL if buf is too small. */
int mpfft_inv_columns_schedule(long n1, long n2, unsigned long depth, unsigned long w, char *buf, size_t len);
int mpfft_profile_end(float *stage_ms, int *calls);

const char *mpfft_strerror(int code);
int mpfft_version(void);

/* splitmix64-seeded xoshiro256** limbs (the benchmark's synthetic operands). */
void mpfft_fill_random(uint64_t *buf, long cnt, uint64_t seed);

#ifdef __cplusplus
}
#endif

#endif /* MPFFT_H */
