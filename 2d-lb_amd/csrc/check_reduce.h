// check_reduce.h -- the health check's record and its reduction, shared by the first passes (k_macro_check, kernels_check.h: flow
// lattices; k_ad_check, kernels_scalar.h: scalar lattices) and the pass that folds their partials (k_check_final, kernels_check.h).
// Every step has a fixed order -- lanes of a wave through cross-lane moves, waves of a workgroup through LDS in index order,
// partials in index order --, so the result does not depend on the order in which workgroups retire.
#pragma once
#include <hip/hip_runtime.h>

struct CheckPartial {
    double sum_rho;                 // over the finite cells
    unsigned long long nonfinite;   // cells whose rho, u or v is not finite
    float max_usq;                  // max u^2 + v^2 (lattice units)
    int pad;
};

namespace {

__device__ __forceinline__ void check_reduce_wave(double &s, unsigned long long &n, float &m)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d);
        n += __shfl_xor(n, d);
        m = fmaxf(m, __shfl_xor(m, d));
    }
}

// Every thread of a workgroup of WAVES waves (one-dimensional) brings its s, n, m: lane 0 of each wave puts the wave's fold into
// LDS, thread 0 folds the WAVES entries in index order and stores the record at *out.
template <int WAVES>
__device__ __forceinline__ void check_reduce_block(double s, unsigned long long n, float m, CheckPartial *out)
{
    __shared__ CheckPartial sh[WAVES];
    check_reduce_wave(s, n, m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = CheckPartial{s, n, m, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        CheckPartial t = sh[0];
        for (int i = 1; i < WAVES; ++i) { t.sum_rho += sh[i].sum_rho; t.nonfinite += sh[i].nonfinite; t.max_usq = fmaxf(t.max_usq, sh[i].max_usq); }
        *out = t;
    }
}

}  // namespace
