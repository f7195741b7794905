// pwsq.hip -- instantiations of the nested negacyclic squaring kernel (pkernels.hpp)
#include "pkernels.hpp"
#include "pdispatch.hpp"

pw_sq_fn pw_get_sqr(int M, int lk, int fuse)
{
    if (M == 10 && lk == 8) return fuse == 2 ? nullptr : fuse ? k_pwsq<10, 8, 1> : k_pwsq<10, 8, 0>;   // l = 1024
    if (M == 18 && lk == 8) return fuse == 2 ? k_pwsq<18, 8, 2> : fuse ? k_pwsq<18, 8, 1> : k_pwsq<18, 8, 0>;   // l = 2048
    if (M == 20 && lk == 9) return fuse == 2 ? k_pwsq<20, 9, 2> : fuse ? k_pwsq<20, 9, 1> : k_pwsq<20, 9, 0>;   // l = 4096
    return nullptr;
}
