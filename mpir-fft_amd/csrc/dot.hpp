// dot.hpp -- sums of products (mpfft_dot_*): the slot-wise accumulation behind the pointwise
// families that form their product in place (k_pwm2, k_pwm, k_pw, k_pointwise).  The nested
// family accumulates inside its pointwise kernel instead (k_pwsa, pkernels.hpp).
// Included by mpfft.hip after kernels.hpp.
#pragma once

// C[slot] <- C[slot] + A[slot] mod 2^N + 1, one workgroup per slot, U limbs per thread (the plan's
// U and threads per coefficient).  Both inputs in any reduced form (coeff.hpp load_coeff); the
// digit sums are below 2^34, far inside wg_norm_multi's bound; the output is the reduced form the
// inverse row passes reload (limbs and +-1 carry masks, top 0).
template <int U>
__global__ __launch_bounds__(1024) void k_slotacc(u64 *digC, u64 *cbC, int *topC, const u64 *digA, const u64 *cbA,
                                                  const int *topA, int l)
{
    Coef sc, sa;
    sc.dig = digC;
    sc.cb = cbC;
    sc.top = topC;
    sa.dig = (u64 *)digA;
    sa.cb = (u64 *)cbA;
    sa.top = (int *)topA;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WG c = wg_ctx();
    const Lds sm = lds_carve<U, 1>(smem, l, 0, c.nw);
    long slot[1] = {(long)blockIdx.x};
    bool keep[1] = {true};
    i64 x[1][2 * U], y[2 * U];
    load_coeff<U>(c, x[0], sc, slot[0], l);
    load_coeff<U>(c, y, sa, slot[0], l);
#pragma unroll
    for (int k = 0; k < 2 * U; ++k) x[0][k] += y[k];
    normalize_store<U, 1>(c, x, slot, keep, false, sc, l, sm);
}
