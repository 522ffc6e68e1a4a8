// GEMM instantiations: activation mode A_CONV3, two-K-group 64-row tile set (gemm_kern.h).
#include "gemm_kern.h"

TAIR_GEMM_SET_TU(A_CONV3, SET_KGROUP, kgroup)
