/* C caller of the mod 2^B + 1 entries: include/mpfft.h + -lmpfft, nothing else.  Takes an
 * efficient size from mpfft_mulmod_next_size(100), then checks mpfft_mulmod_ex on (0, 5), on
 * (2^B, 2^B) and on a seeded pair, and mpfft_sqrmod_ex on the seeded operand, against the full
 * product of mpfft_mul_ex folded here at 2^B == -1 (low half minus high half, plus M when that is
 * negative).  Built by __graft_entry__.build() (tests/c_mulmod/Makefile), run as a child process
 * by tests/test_gpu_mulmod.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

/* r[0 .. L] = p[0 .. 2L) mod 2^(64 L) + 1 */
static void fold(uint64_t *r, const uint64_t *p, long L)
{
    unsigned borrow = 0;
    long i;
    for (i = 0; i < L; ++i) {
        const uint64_t a = p[i], b = p[L + i], d = a - b;
        r[i] = d - borrow;
        borrow = (a < b) || (d < borrow);
    }
    r[L] = 0;
    if (borrow) { /* lo - hi + 2^B + 1: the wrapped limbs already hold lo - hi + 2^B */
        for (i = 0; i < L && ++r[i] == 0; ++i)
            ;
        if (i == L) r[L] = 1;
    }
}

static int check(const char *what, const uint64_t *got, const uint64_t *want, long L)
{
    long i;
    for (i = 0; i <= L; ++i)
        if (got[i] != want[i]) {
            printf("FAIL: %s differs at limb %ld of %ld\n", what, i, L + 1);
            return 1;
        }
    return 0;
}

int main(void)
{
    long L = 0, i;
    unsigned long depth = 0, w = 0, d2 = 0, w2 = 0;
    int rc;
    if (mpfft_version() < 4) {
        printf("FAIL: mpfft_version() = %d, the mod 2^B + 1 entries need 4\n", mpfft_version());
        return 1;
    }
    if ((rc = mpfft_mulmod_next_size(100, &L, &depth, &w)) || L < 100 || mpfft_mulmod_check_params(L, depth, w)) {
        printf("FAIL: mpfft_mulmod_next_size: rc %d, L %ld depth %lu w %lu\n", rc, L, depth, w);
        return 1;
    }
    uint64_t *a = calloc(L + 1, 8), *b = calloc(L + 1, 8), *r = calloc(L + 1, 8), *want = calloc(L + 1, 8);
    uint64_t *full = calloc(2 * L, 8);
    if (!a || !b || !r || !want || !full) return 1;

    b[0] = 5; /* 0 * 5 */
    memset(r, 0xa5, (L + 1) * 8);
    if ((rc = mpfft_mulmod_ex(r, a, b, L, depth, w))) goto fail;
    if (check("0 * 5", r, want, L)) return 1;

    b[0] = 0; /* 2^B * 2^B = (-1)^2 = 1 */
    a[L] = b[L] = 1;
    want[0] = 1;
    memset(r, 0xa5, (L + 1) * 8);
    if ((rc = mpfft_mulmod_ex(r, a, b, L, depth, w))) goto fail;
    if (check("2^B * 2^B", r, want, L)) return 1;

    a[L] = b[L] = 0; /* a seeded pair against the folded full product */
    mpfft_fill_random(a, L, 0x5a17);
    mpfft_fill_random(b, L, 0x17a5);
    if ((rc = mpfft_choose(L, L, &d2, &w2)) || (rc = mpfft_mul_ex(full, a, L, b, L, d2, w2))) goto fail;
    fold(want, full, L);
    memset(r, 0xa5, (L + 1) * 8);
    if ((rc = mpfft_mulmod_ex(r, a, b, L, depth, w))) goto fail;
    if (check("seeded a * b", r, want, L)) return 1;

    if ((rc = mpfft_mul_ex(full, a, L, a, L, d2, w2))) goto fail;
    fold(want, full, L);
    memset(r, 0xa5, (L + 1) * 8);
    if ((rc = mpfft_sqrmod_ex(r, a, L, depth, w))) goto fail;
    if (check("seeded a^2", r, want, L)) return 1;

    a[L] = 1; /* not reduced: refused */
    if (mpfft_mulmod_ex(r, a, b, L, depth, w) != MPFFT_EINVAL) {
        printf("FAIL: a non-reduced operand was accepted\n");
        return 1;
    }
    for (i = 0; i <= L; ++i) a[i] = 0;
    (void)mpfft_release();
    free(a); free(b); free(r); free(want); free(full);
    printf("OK\n");
    return 0;
fail:
    printf("FAIL: %s\n", mpfft_strerror(rc));
    return 1;
}
