/* C caller of the signed sums of products: include/mpfft.h + -lmpfft, nothing else.  a b - c d and
 * -(a b) of seeded 3000 x 2000-limb operands through mpfft_sdot_auto, against the products of
 * mpfft_mul_auto subtracted here limb by limb (two's complement in n1 + n2 + 1 limbs); the
 * MPFFT_EINVAL for a mask bit at or above K; the version.  Built by __graft_entry__.build()
 * (tests/c_sdot/Makefile), run as a child process by tests/test_gpu_sdot.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

/* s[0 .. n] += p[0 .. n) or -= p[0 .. n), mod 2^(64 (n + 1)) */
static void acc_into(uint64_t *s, const uint64_t *p, long n, int sub)
{
    unsigned c = 0;
    long i;
    for (i = 0; i <= n; ++i) {
        const uint64_t v = i < n ? p[i] : 0;
        if (sub) {
            const uint64_t x = s[i] - v, y = x - c;
            c = (s[i] < v) || (x < c);
            s[i] = y;
        } else {
            const uint64_t x = s[i] + v, y = x + c;
            c = (x < v) || (y < x);
            s[i] = y;
        }
    }
}

static int check(const char *what, const uint64_t *got, const uint64_t *want, long n)
{
    long i;
    for (i = 0; i < n; ++i)
        if (got[i] != want[i]) {
            printf("FAIL: %s differs at limb %ld of %ld\n", what, i, n);
            return 1;
        }
    return 0;
}

int main(void)
{
    const long n1 = 3000, n2 = 2000, nr = n1 + n2 + 1;
    const uint64_t *pa[2], *pb[2];
    uint64_t *a[2], *b[2];
    int rc, k;
    if (mpfft_version() < 9) {
        printf("FAIL: mpfft_version() = %d, the sdot entries need 9\n", mpfft_version());
        return 1;
    }
    uint64_t *r = calloc(nr, 8), *want = calloc(nr, 8), *prod = calloc(n1 + n2, 8);
    if (!r || !want || !prod) return 1;
    for (k = 0; k < 2; ++k) {
        a[k] = malloc(n1 * 8);
        b[k] = malloc(n2 * 8);
        if (!a[k] || !b[k]) return 1;
        mpfft_fill_random(a[k], n1, 0x5d070 + k);
        mpfft_fill_random(b[k], n2, 0x5d170 + k);
        pa[k] = a[k];
        pb[k] = b[k];
    }
    if (mpfft_sdot_check_params(2, 4, n1, n2, 9, 64) != MPFFT_EINVAL || mpfft_sdot_auto(r, 2, 4, pa, pb, n1, n2) != MPFFT_EINVAL
        || mpfft_sdot_auto(r, 1, 2, pa, pb, n1, n2) != MPFFT_EINVAL) {
        printf("FAIL: a mask bit at or above K accepted\n");
        return 1;
    }
    /* a0 b0 - a1 b1 */
    if ((rc = mpfft_mul_auto(prod, a[0], n1, b[0], n2))) goto fail;
    acc_into(want, prod, n1 + n2, 0);
    if ((rc = mpfft_mul_auto(prod, a[1], n1, b[1], n2))) goto fail;
    acc_into(want, prod, n1 + n2, 1);
    memset(r, 0xa5, nr * 8);
    if ((rc = mpfft_sdot_auto(r, 2, 2, pa, pb, n1, n2))) goto fail;
    if (check("a b - c d", r, want, nr)) return 1;
    /* -(a0 b0) */
    memset(want, 0, nr * 8);
    if ((rc = mpfft_mul_auto(prod, a[0], n1, b[0], n2))) goto fail;
    acc_into(want, prod, n1 + n2, 1);
    memset(r, 0xa5, nr * 8);
    if ((rc = mpfft_sdot_auto(r, 1, 1, pa, pb, n1, n2))) goto fail;
    if (check("-(a b)", r, want, nr)) return 1;
    if (r[nr - 1] != ~(uint64_t)0) {
        printf("FAIL: the top limb of -(a b) is not all ones\n");
        return 1;
    }
    printf("sdot_caller: a b - c d and -(a b) at %ld x %ld limbs\nOK\n", n1, n2);
    return 0;
fail:
    printf("FAIL: rc %d (%s)\n", rc, mpfft_strerror(rc));
    return 1;
}
