/* C caller of the precomputed-operand entries: include/mpfft.h + -lmpfft, nothing else.  Caches a
 * seeded operand with mpfft_precomp_create (depth 9, w 2, 120 x 97 limbs), multiplies two other
 * operands by it with mpfft_mul_precomp_ex, compares each with mpfft_mul_ex limb for limb, checks
 * that another operand size is refused, and prints OK.  Built by __graft_entry__.build()
 * (tests/c_precomp/Makefile), run as a child process by tests/test_gpu_precomp.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

int main(void)
{
    enum { N1 = 120, N2 = 97 };
    const unsigned long depth = 9, w = 2;
    uint64_t a[N1], b[N2], pr[N1 + N2], mu[N1 + N2];
    mpfft_pre *pre = NULL;
    int rc;
    if (mpfft_version() < 5) {
        printf("FAIL: mpfft_version() = %d, the precomputed-operand entries need 5\n", mpfft_version());
        return 1;
    }
    mpfft_fill_random(b, N2, 0x9b1);
    if ((rc = mpfft_precomp_create(&pre, b, N2, N1, depth, w)) || !pre) {
        printf("FAIL: mpfft_precomp_create: %s\n", mpfft_strerror(rc));
        return 1;
    }
    for (int k = 0; k < 2; ++k) {
        mpfft_fill_random(a, N1, 0x5a17 + k);
        memset(pr, 0xa5, sizeof pr);
        memset(mu, 0x5a, sizeof mu);
        if ((rc = mpfft_mul_precomp_ex(pr, a, N1, pre))) {
            printf("FAIL: mpfft_mul_precomp_ex: %s\n", mpfft_strerror(rc));
            return 1;
        }
        if ((rc = mpfft_mul_ex(mu, a, N1, b, N2, depth, w))) {
            printf("FAIL: mpfft_mul_ex: %s\n", mpfft_strerror(rc));
            return 1;
        }
        if (memcmp(pr, mu, sizeof pr)) {
            int i = 0;
            while (pr[i] == mu[i]) ++i;
            printf("FAIL: product %d against the cache differs from a * b at limb %d\n", k, i);
            return 1;
        }
    }
    if (mpfft_mul_precomp_ex(pr, a, N1 - 1, pre) != MPFFT_EINVAL) {
        printf("FAIL: another n1 was not refused\n");
        return 1;
    }
    mpfft_precomp_destroy(pre);
    (void)mpfft_release();
    printf("OK\n");
    return 0;
}
