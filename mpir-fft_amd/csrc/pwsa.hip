// pwsa.hip -- instantiations of the accumulating nested negacyclic pointwise kernel (pkernels.hpp):
// k_pwsa<M, lk, fuse>, C <- C + A B, the same instance table as k_pwss (pwss.hip)
#include "pkernels.hpp"
#include "pdispatch.hpp"

pw_acc_fn pw_get_acc(int M, int lk, int fuse)
{
    if (M == 10 && lk == 8) return fuse == 2 ? nullptr : fuse ? k_pwsa<10, 8, 1> : k_pwsa<10, 8, 0>;   // l = 1024
    if (M == 18 && lk == 8) return fuse == 2 ? k_pwsa<18, 8, 2> : fuse ? k_pwsa<18, 8, 1> : k_pwsa<18, 8, 0>;   // l = 2048
    if (M == 20 && lk == 9) return fuse == 2 ? k_pwsa<20, 9, 2> : fuse ? k_pwsa<20, 9, 1> : k_pwsa<20, 9, 0>;   // l = 4096
    return nullptr;
}
