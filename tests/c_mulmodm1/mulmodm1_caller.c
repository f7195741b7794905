/* C caller of the mod 2^B - 1 entries: include/mpfft.h + -lmpfft, nothing else.  Takes an
 * efficient size from mpfft_mulmodm1_next_size(100), then checks mpfft_mulmodm1_ex on (0, 5), on
 * (all-ones, 5) and (2^B - 2, 2^B - 2) and on a seeded pair, and mpfft_sqrmodm1_ex on the seeded
 * operand, against the full product of mpfft_mul_ex folded here at 2^B == 1 (low half plus high
 * half with the end-around carry, all-ones stored as 0).  Built by __graft_entry__.build()
 * (tests/c_mulmodm1/Makefile), run as a child process by tests/test_gpu_mulmodm1.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

/* r[0 .. L) = p[0 .. 2L) mod 2^(64 L) - 1, fully reduced */
static void fold(uint64_t *r, const uint64_t *p, long L)
{
    unsigned carry = 0;
    long i;
    for (i = 0; i < L; ++i) {
        const uint64_t s = p[i] + p[L + i], t = s + carry;
        carry = (s < p[i]) || (t < s);
        r[i] = t;
    }
    if (carry) /* lo + hi - 2^B + 1 <= 2^B - 1: no second carry */
        for (i = 0; i < L && ++r[i] == 0; ++i)
            ;
    for (i = 0; i < L && r[i] == ~(uint64_t)0; ++i)
        ;
    if (i == L) memset(r, 0, (size_t)L * 8);
}

static int check(const char *what, const uint64_t *got, const uint64_t *want, long L)
{
    long i;
    for (i = 0; i < L; ++i)
        if (got[i] != want[i]) {
            printf("FAIL: %s differs at limb %ld of %ld\n", what, i, L);
            return 1;
        }
    return 0;
}

int main(void)
{
    long L = 0;
    unsigned long depth = 0, w = 0, d2 = 0, w2 = 0;
    int rc;
    if (mpfft_version() < 6) {
        printf("FAIL: mpfft_version() = %d, the mod 2^B - 1 entries need 6\n", mpfft_version());
        return 1;
    }
    if ((rc = mpfft_mulmodm1_next_size(100, &L, &depth, &w)) || L < 100 || mpfft_mulmodm1_check_params(L, depth, w)) {
        printf("FAIL: mpfft_mulmodm1_next_size: rc %d, L %ld depth %lu w %lu\n", rc, L, depth, w);
        return 1;
    }
    uint64_t *a = calloc(L, 8), *b = calloc(L, 8), *r = calloc(L, 8), *want = calloc(L, 8);
    uint64_t *full = calloc(2 * L, 8);
    if (!a || !b || !r || !want || !full) return 1;

    b[0] = 5; /* 0 * 5 */
    memset(r, 0xa5, L * 8);
    if ((rc = mpfft_mulmodm1_ex(r, a, b, L, depth, w))) goto fail;
    if (check("0 * 5", r, want, L)) return 1;

    memset(a, 0xff, L * 8); /* all-ones is 0 mod M */
    memset(r, 0xa5, L * 8);
    if ((rc = mpfft_mulmodm1_ex(r, a, b, L, depth, w))) goto fail;
    if (check("all-ones * 5", r, want, L)) return 1;

    a[0] -= 1; /* (M - 1)^2 = (-1)^2 = 1 */
    want[0] = 1;
    memset(r, 0xa5, L * 8);
    if ((rc = mpfft_sqrmodm1_ex(r, a, L, depth, w))) goto fail;
    if (check("(M - 1)^2", r, want, L)) return 1;

    mpfft_fill_random(a, L, 0x5a17); /* a seeded pair against the folded full product */
    mpfft_fill_random(b, L, 0x17a5);
    if ((rc = mpfft_choose(L, L, &d2, &w2)) || (rc = mpfft_mul_ex(full, a, L, b, L, d2, w2))) goto fail;
    fold(want, full, L);
    memset(r, 0xa5, L * 8);
    if ((rc = mpfft_mulmodm1_ex(r, a, b, L, depth, w))) goto fail;
    if (check("seeded a * b", r, want, L)) return 1;

    if ((rc = mpfft_mul_ex(full, a, L, a, L, d2, w2))) goto fail;
    fold(want, full, L);
    memset(r, 0xa5, L * 8);
    if ((rc = mpfft_sqrmodm1_ex(r, a, L, depth, w))) goto fail;
    if (check("seeded a^2", r, want, L)) return 1;

    (void)mpfft_release();
    free(a); free(b); free(r); free(want); free(full);
    printf("OK\n");
    return 0;
fail:
    printf("FAIL: %s\n", mpfft_strerror(rc));
    return 1;
}
