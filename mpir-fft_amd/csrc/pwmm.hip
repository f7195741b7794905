// pwmm.hip -- instantiations of the matrix-product form of the nested negacyclic pointwise kernel
// (pkernels.hpp): k_pwmm<M, lk, acc>, C (+)= sum of kk products of cached records
#include "pkernels.hpp"
#include "pdispatch.hpp"
#include "../../include/mpfft.h"

static_assert(PW_MM_MAX == MPFFT_MM_MAX, "the kernel's term bound is the entry's");

pw_mm_fn pw_get_mm(int M, int lk, bool acc)
{
    if (M == 10 && lk == 8) return acc ? k_pwmm<10, 8, true> : k_pwmm<10, 8, false>;   // l = 1024
    if (M == 18 && lk == 8) return acc ? k_pwmm<18, 8, true> : k_pwmm<18, 8, false>;   // l = 2048
    if (M == 20 && lk == 9) return acc ? k_pwmm<20, 9, true> : k_pwmm<20, 9, false>;   // l = 4096
    return nullptr;
}
