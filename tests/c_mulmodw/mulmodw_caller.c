/* C caller of the mod 2^B + 1 entries with the low-word CRT: include/mpfft.h + -lmpfft, nothing
 * else.  At the Fermat size L = 1024 (B = 2^16) it takes (depth, w) from mpfft_mulmodw_choose,
 * checks that mpfft_mulmod_check_params refuses the pair (the pieces are past the plain bound),
 * then checks mpfft_mulmodw_ex on (0, 5), on (2^B, 2^B), on (2^B, b) and on a seeded pair, and
 * mpfft_sqrmodw_ex on the seeded operand, against mpfft_mulmod_ex at mpfft_mulmod_choose's pair;
 * the same seeded pair once more at an efficient size from mpfft_mulmodw_next_size(100).  Built by
 * __graft_entry__.build() (tests/c_mulmodw/Makefile), run as a child process by
 * tests/test_gpu_mulmodw.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

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

/* mpfft_mulmodw_ex (b null: mpfft_sqrmodw_ex) against the plain family at its own pair */
static int both(const char *what, const uint64_t *a, const uint64_t *b, long L, unsigned long depth, unsigned long w,
                uint64_t *r, uint64_t *want)
{
    unsigned long d0 = 0, w0 = 0;
    int rc;
    if ((rc = mpfft_mulmod_choose(L, &d0, &w0))) goto fail;
    memset(r, 0xa5, (L + 1) * 8);
    memset(want, 0x5a, (L + 1) * 8);
    if ((rc = b ? mpfft_mulmod_ex(want, a, b, L, d0, w0) : mpfft_sqrmod_ex(want, a, L, d0, w0))) goto fail;
    if ((rc = b ? mpfft_mulmodw_ex(r, a, b, L, depth, w) : mpfft_sqrmodw_ex(r, a, L, depth, w))) goto fail;
    return check(what, r, want, L);
fail:
    printf("FAIL: %s: %s\n", what, mpfft_strerror(rc));
    return 1;
}

int main(void)
{
    long L = 1024, L2 = 0;
    unsigned long depth = 0, w = 0, d2 = 0, w2 = 0;
    int rc;
    if (mpfft_version() < 7) {
        printf("FAIL: mpfft_version() = %d, the low-word CRT entries need 7\n", mpfft_version());
        return 1;
    }
    if ((rc = mpfft_mulmodw_choose(L, &depth, &w)) || mpfft_mulmodw_check_params(L, depth, w)) {
        printf("FAIL: mpfft_mulmodw_choose: rc %d, depth %lu w %lu\n", rc, depth, w);
        return 1;
    }
    if (mpfft_mulmod_check_params(L, depth, w) != MPFFT_ETOOBIG) {
        printf("FAIL: depth %lu w %lu at L %ld is within the plain bound\n", depth, w, L);
        return 1;
    }
    if ((rc = mpfft_mulmodw_next_size(100, &L2, &d2, &w2)) || L2 < 100 || L2 > L || mpfft_mulmodw_check_params(L2, d2, w2)) {
        printf("FAIL: mpfft_mulmodw_next_size: rc %d, L %ld depth %lu w %lu\n", rc, L2, d2, w2);
        return 1;
    }
    uint64_t *a = calloc(L + 1, 8), *b = calloc(L + 1, 8), *r = calloc(L + 1, 8), *want = calloc(L + 1, 8);
    if (!a || !b || !r || !want) return 1;

    b[0] = 5; /* 0 * 5 */
    if (both("0 * 5", a, b, L, depth, w, r, want)) return 1;
    b[0] = 0; /* 2^B * 2^B = (-1)^2 = 1 */
    a[L] = b[L] = 1;
    if (both("2^B * 2^B", a, b, L, depth, w, r, want)) return 1;
    if (r[0] != 1 || r[L] != 0) {
        printf("FAIL: 2^B * 2^B is not 1\n");
        return 1;
    }
    b[L] = 0; /* 2^B * b = M - b */
    mpfft_fill_random(b, L, 0x17a5);
    if (both("2^B * b", a, b, L, depth, w, r, want)) return 1;
    a[L] = 0; /* a seeded pair */
    mpfft_fill_random(a, L, 0x5a17);
    if (both("seeded a * b", a, b, L, depth, w, r, want)) return 1;
    if (both("seeded a^2", a, NULL, L, depth, w, r, want)) return 1;
    a[L2] = b[L2] = 0; /* the low L2 limbs at the efficient size */
    if (both("seeded a * b at next_size", a, b, L2, d2, w2, r, want)) return 1;

    a[L2] = 1; /* not reduced: refused */
    if (mpfft_mulmodw_ex(r, a, b, L2, d2, w2) != MPFFT_EINVAL) {
        printf("FAIL: a non-reduced operand was accepted\n");
        return 1;
    }
    (void)mpfft_release();
    free(a); free(b); free(r); free(want);
    printf("OK\n");
    return 0;
}
