/* C caller of the squaring entry: include/mpfft.h + -lmpfft, nothing else.  Squares a seeded
 * operand with mpfft_sqr_ex (depth 9, w 2, n 120), compares with mpfft_mul_ex(a, a) limb for limb
 * and prints OK.  Built by __graft_entry__.build() (tests/c_sqr/Makefile), run as a child
 * process by tests/test_gpu_sqr.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

int main(void)
{
    enum { N = 120 };
    const unsigned long depth = 9, w = 2;
    uint64_t a[N], sq[2 * N], mu[2 * N];
    int rc;
    if (mpfft_version() < 3) {
        printf("FAIL: mpfft_version() = %d, the squaring entries need 3\n", mpfft_version());
        return 1;
    }
    mpfft_fill_random(a, N, 0x5a17);
    memset(sq, 0xa5, sizeof sq);
    memset(mu, 0x5a, sizeof mu);
    if ((rc = mpfft_sqr_ex(sq, a, N, depth, w))) {
        printf("FAIL: mpfft_sqr_ex: %s\n", mpfft_strerror(rc));
        return 1;
    }
    if ((rc = mpfft_mul_ex(mu, a, N, a, N, depth, w))) {
        printf("FAIL: mpfft_mul_ex: %s\n", mpfft_strerror(rc));
        return 1;
    }
    if (memcmp(sq, mu, sizeof sq)) {
        int i = 0;
        while (sq[i] == mu[i]) ++i;
        printf("FAIL: square differs from a * a at limb %d\n", i);
        return 1;
    }
    (void)mpfft_release();
    printf("OK\n");
    return 0;
}
