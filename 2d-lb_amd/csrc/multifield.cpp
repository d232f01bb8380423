// multifield.cpp -- the translation unit of coupled scalar lattices: instantiates and launches the kernels of kernels_multifield.h
// (multifield_launch.h).
#include "kernels_multifield.h"

namespace {

template <int BC, int NF>
void mf_step_go(bool store_rho, dim3 grid, dim3 block, hipStream_t st, const MfArgs &m)
{
    if (store_rho) hipLaunchKernelGGL((k_mf_step<BC, NF, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_mf_step<BC, NF, false>), grid, block, 0, st, m);
}

template <int BC>
void mf_step_nf(int nf, bool store_rho, dim3 grid, dim3 block, hipStream_t st, const MfArgs &m)
{
    if (nf == 1) mf_step_go<BC, 1>(store_rho, grid, block, st, m);
    else if (nf == 2) mf_step_go<BC, 2>(store_rho, grid, block, st, m);
    else if (nf == 3) mf_step_go<BC, 3>(store_rho, grid, block, st, m);
    else mf_step_go<BC, 4>(store_rho, grid, block, st, m);
}

}  // namespace

void lbk_mf_step(int bc, int nf, bool store_rho, hipStream_t st, const MfArgs &m)
{
    const StepArgs &a = m.a[0];
    const dim3 block(64, 4), grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4));
    if (bc == LB_BC_PERIODIC) mf_step_nf<LB_BC_PERIODIC>(nf, store_rho, grid, block, st, m);
    else mf_step_nf<LB_BC_BOX>(nf, store_rho, grid, block, st, m);
}

void lbk_mf_move_bcs(hipStream_t st, const StepArgs &a, float *f)
{
    const int n = a.nx > a.ny ? a.nx : a.ny;
    hipLaunchKernelGGL(k_mf_move_bcs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f);
}

void lbk_mf_collide(int nf, hipStream_t st, const MfArgs &m)
{
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.nx + 255) / 256), (unsigned)a.ny), block(256);
    if (nf == 1) hipLaunchKernelGGL(k_mf_collide<1>, grid, block, 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mf_collide<2>, grid, block, 0, st, m);
    else if (nf == 3) hipLaunchKernelGGL(k_mf_collide<3>, grid, block, 0, st, m);
    else hipLaunchKernelGGL(k_mf_collide<4>, grid, block, 0, st, m);
}
