/* C caller of the small matrix products: include/mpfft.h + -lmpfft, nothing else.  A 2x2 by 2x2 product
 * of seeded 3000- and 2000-limb entries through mpfft_matmul_ex (with mpfft_dot_choose's parameters) and
 * mpfft_matmul_auto, one operand at two places of X, against mpfft_dot_auto entry by entry; a 2x3 by 3x1
 * product the same way; and the status codes for a dimension of 0 and of MPFFT_MM_MAX + 1.  Built by
 * __graft_entry__.build() (tests/c_matmul/Makefile), run as a child process by tests/test_gpu_matmul.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mpfft.h"

static int check(const char *what, int e, const uint64_t *got, const uint64_t *want, long n)
{
    long i;
    for (i = 0; i < n; ++i)
        if (got[i] != want[i]) {
            printf("FAIL: %s entry %d differs at limb %ld of %ld\n", what, e, i, n);
            return 1;
        }
    return 0;
}

/* X (m x k) Y (k x p) through both host entries against mpfft_dot_auto on each entry's k terms */
static int product(const char *what, int m, int k, int p, const uint64_t *const *x, const uint64_t *const *y, long n1, long n2)
{
    const long nr = n1 + n2 + 1;
    unsigned long depth = 0, w = 0;
    uint64_t *r[MPFFT_MM_MAX * MPFFT_MM_MAX], *want = malloc(nr * 8);
    const uint64_t *ta[MPFFT_MM_MAX], *tb[MPFFT_MM_MAX];
    int rc, i, j, t, e, pass;
    if (!want) return 1;
    for (e = 0; e < m * p; ++e)
        if (!(r[e] = malloc(nr * 8))) return 1;
    if ((rc = mpfft_dot_choose(k, n1, n2, &depth, &w)) || (rc = mpfft_matmul_check_params(m, k, p, n1, n2, depth, w))) goto fail;
    for (pass = 0; pass < 2; ++pass) {
        for (e = 0; e < m * p; ++e) memset(r[e], 0xa5, nr * 8);
        rc = pass ? mpfft_matmul_auto(r, m, k, p, x, y, n1, n2) : mpfft_matmul_ex(r, m, k, p, x, y, n1, n2, depth, w);
        if (rc) goto fail;
        for (i = 0; i < m; ++i)
            for (j = 0; j < p; ++j) {
                for (t = 0; t < k; ++t) {
                    ta[t] = x[i * k + t];
                    tb[t] = y[t * p + j];
                }
                if ((rc = mpfft_dot_auto(want, k, ta, tb, n1, n2))) goto fail;
                if (check(what, i * p + j, r[i * p + j], want, nr)) return 1;
            }
    }
    for (e = 0; e < m * p; ++e) free(r[e]);
    free(want);
    return 0;
fail:
    printf("FAIL: %s: rc %d (%s)\n", what, rc, mpfft_strerror(rc));
    return 1;
}

int main(void)
{
    const long n1 = 3000, n2 = 2000;
    uint64_t *a[6], *b[4];
    const uint64_t *x[6], *y[4];
    int k;
    if (mpfft_version() < 10) {
        printf("FAIL: mpfft_version() = %d, the matmul entries need 10\n", mpfft_version());
        return 1;
    }
    if (mpfft_matmul_check_params(0, 2, 2, n1, n2, 9, 64) != MPFFT_EINVAL || mpfft_matmul_check_params(2, MPFFT_MM_MAX + 1, 2, n1, n2, 9, 64) != MPFFT_EINVAL
        || mpfft_matmul_check_params(2, 2, -1, n1, n2, 9, 64) != MPFFT_EINVAL || mpfft_matmul_workspace_bytes(2, 2, 5, n1, n2, 9, 64) != 0) {
        printf("FAIL: a dimension outside [1, %d] accepted\n", MPFFT_MM_MAX);
        return 1;
    }
    for (k = 0; k < 6; ++k) {
        if (!(a[k] = malloc(n1 * 8))) return 1;
        mpfft_fill_random(a[k], n1, 0x3a70 + k);
    }
    for (k = 0; k < 4; ++k) {
        if (!(b[k] = malloc(n2 * 8))) return 1;
        mpfft_fill_random(b[k], n2, 0x3b70 + k);
    }
    /* X = [a0 a1; a2 a0]: a0 appears twice */
    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[0];
    for (k = 0; k < 4; ++k) y[k] = b[k];
    if (product("2x2 by 2x2", 2, 2, 2, x, y, n1, n2)) return 1;
    for (k = 0; k < 6; ++k) x[k] = a[k];
    if (product("2x3 by 3x1", 2, 3, 1, x, y, n1, n2)) return 1;
    printf("matmul_caller: 2x2 by 2x2 and 2x3 by 3x1, %ld- and %ld-limb entries\nOK\n", n1, n2);
    return 0;
}
