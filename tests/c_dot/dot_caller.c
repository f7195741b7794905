/* C caller of the sums of products: include/mpfft.h + -lmpfft, nothing else.  A three-term sum of
 * seeded 3000 x 2000-limb products through mpfft_dot_ex (with mpfft_dot_choose's parameters) and
 * mpfft_dot_auto, one operand shared by two terms, against the three products of mpfft_mul_auto
 * added here limb by limb; then 64 all-ones terms (the top limb is 63) and the status codes for
 * K = 0 and K = 65.  Built by __graft_entry__.build() (tests/c_dot/Makefile), run as a child
 * process by tests/test_gpu_dot.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

/* s[0 .. n] += p[0 .. n) */
static void add_into(uint64_t *s, const uint64_t *p, long n)
{
    unsigned carry = 0;
    long i;
    for (i = 0; i < n; ++i) {
        const uint64_t x = s[i] + p[i], y = x + carry;
        carry = (x < p[i]) || (y < x);
        s[i] = y;
    }
    s[n] += carry;
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
    enum { K = 3 };
    const long n1 = 3000, n2 = 2000, nr = n1 + n2 + 1;
    unsigned long depth = 0, w = 0;
    const uint64_t *pa[MPFFT_DOT_MAX], *pb[MPFFT_DOT_MAX];
    uint64_t *a[K], *b[K];
    long i;
    int rc, k;
    if (mpfft_version() < 8) {
        printf("FAIL: mpfft_version() = %d, the dot entries need 8\n", mpfft_version());
        return 1;
    }
    if (mpfft_dot_check_params(0, n1, n2, 9, 64) != MPFFT_EINVAL || mpfft_dot_check_params(MPFFT_DOT_MAX + 1, n1, n2, 9, 64) != MPFFT_EINVAL) {
        printf("FAIL: K = 0 or K = %d accepted\n", MPFFT_DOT_MAX + 1);
        return 1;
    }
    if ((rc = mpfft_dot_choose(K, n1, n2, &depth, &w)) || mpfft_dot_check_params(K, n1, n2, depth, w)) {
        printf("FAIL: mpfft_dot_choose: rc %d, depth %lu w %lu\n", rc, depth, w);
        return 1;
    }
    uint64_t *r = calloc(nr, 8), *want = calloc(nr, 8), *prod = calloc(n1 + n2, 8);
    if (!r || !want || !prod) return 1;
    for (k = 0; k < K; ++k) {
        a[k] = malloc(n1 * 8);
        b[k] = malloc(n2 * 8);
        if (!a[k] || !b[k]) return 1;
        mpfft_fill_random(a[k], n1, 0xd070 + k);
        mpfft_fill_random(b[k], n2, 0xd170 + k);
    }
    /* terms (a0, b0), (a1, b1), (a0, b2): a0 appears twice */
    pa[0] = a[0]; pa[1] = a[1]; pa[2] = a[0];
    pb[0] = b[0]; pb[1] = b[1]; pb[2] = b[2];
    for (k = 0; k < K; ++k) {
        if ((rc = mpfft_mul_auto(prod, pa[k], n1, pb[k], n2))) goto fail;
        add_into(want, prod, n1 + n2);
    }
    memset(r, 0xa5, nr * 8);
    if ((rc = mpfft_dot_ex(r, K, pa, pb, n1, n2, depth, w))) goto fail;
    if (check("mpfft_dot_ex", r, want, nr)) return 1;
    memset(r, 0xa5, nr * 8);
    if ((rc = mpfft_dot_auto(r, K, pa, pb, n1, n2))) goto fail;
    if (check("mpfft_dot_auto", r, want, nr)) return 1;

    /* 64 (2^(64 n2) - 1)^2 = 64 2^(128 n2) - 128 2^(64 n2) + 64 */
    for (i = 0; i < n2; ++i) b[0][i] = ~(uint64_t)0;
    for (k = 0; k < MPFFT_DOT_MAX; ++k) pa[k] = pb[k] = b[0];
    if ((rc = mpfft_dot_auto(r, MPFFT_DOT_MAX, pa, pb, n2, n2))) goto fail;
    memset(want, 0, nr * 8);
    want[0] = 64;
    for (i = 1; i < n2; ++i) want[i] = 0;
    want[n2] = (uint64_t)0 - 128;
    for (i = n2 + 1; i < 2 * n2; ++i) want[i] = ~(uint64_t)0;
    want[2 * n2] = 63;
    if (check("64 all-ones terms", r, want, 2 * n2 + 1)) return 1;
    printf("dot_caller: depth %lu w %lu, K = %d and K = %d\nOK\n", depth, w, K, MPFFT_DOT_MAX);
    return 0;
fail:
    printf("FAIL: rc %d (%s)\n", rc, mpfft_strerror(rc));
    return 1;
}
