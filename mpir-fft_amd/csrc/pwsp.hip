// pwsp.hip -- instantiations of the cached-operand forms of the nested negacyclic pointwise
// kernel (pkernels.hpp): k_pwsx (B's slots -> cache records) and k_pwsp (A times the records)
#include "pkernels.hpp"
#include "pdispatch.hpp"

pw_pre_fn pw_get_pre(int M, int lk, int fuse)
{
    if (M == 10 && lk == 8) return fuse == 2 ? nullptr : fuse ? k_pwsx<10, 8, 1> : k_pwsx<10, 8, 0>;   // l = 1024
    if (M == 18 && lk == 8) return fuse == 2 ? k_pwsx<18, 8, 2> : fuse ? k_pwsx<18, 8, 1> : k_pwsx<18, 8, 0>;   // l = 2048
    if (M == 20 && lk == 9) return fuse == 2 ? k_pwsx<20, 9, 2> : fuse ? k_pwsx<20, 9, 1> : k_pwsx<20, 9, 0>;   // l = 4096
    return nullptr;
}

pw_mulpre_fn pw_get_mulpre(int M, int lk, int fuse)
{
    if (M == 10 && lk == 8) return fuse == 2 ? nullptr : fuse ? k_pwsp<10, 8, 1> : k_pwsp<10, 8, 0>;   // l = 1024
    if (M == 18 && lk == 8) return fuse == 2 ? k_pwsp<18, 8, 2> : fuse ? k_pwsp<18, 8, 1> : k_pwsp<18, 8, 0>;   // l = 2048
    if (M == 20 && lk == 9) return fuse == 2 ? k_pwsp<20, 9, 2> : fuse ? k_pwsp<20, 9, 1> : k_pwsp<20, 9, 0>;   // l = 4096
    return nullptr;
}

size_t pw_pre_record_bytes(int M, int K) { return pw_pre_slot_bytes(M, K); }
