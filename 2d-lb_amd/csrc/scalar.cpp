// scalar.cpp -- the translation unit of scalar lattices: instantiates and launches the kernels of kernels_scalar.h (scalar_launch.h).
#include "kernels_scalar.h"

namespace {

dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }

template <int BC>
void ad_step_go(bool react, bool store_rho, dim3 grid, dim3 block, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    if (react) {
        if (store_rho) hipLaunchKernelGGL((k_ad_step<BC, true, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_ad_step<BC, true, false>), grid, block, 0, st, a, e);
    } else {
        if (store_rho) hipLaunchKernelGGL((k_ad_step<BC, false, true>), grid, block, 0, st, a, e);
        else hipLaunchKernelGGL((k_ad_step<BC, false, false>), grid, block, 0, st, a, e);
    }
}

template <int BC, bool REACT, bool RHO>
void ad_tile_go(int shape, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    with_tile_shape(shape, a.nx, a.ny, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_ad_tile4<BC, REACT, RHO, T::TW, T::TH, T::CPT>), t.grid, t.block, 0, st, a, e, t.tiles_x, t.n_tiles);
    });
}

template <int BC>
void ad_tile_bc(bool react, bool store_rho, int shape, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    if (react) {
        if (store_rho) ad_tile_go<BC, true, true>(shape, st, a, e);
        else ad_tile_go<BC, true, false>(shape, st, a, e);
    } else {
        if (store_rho) ad_tile_go<BC, false, true>(shape, st, a, e);
        else ad_tile_go<BC, false, false>(shape, st, a, e);
    }
}

}  // namespace

void lbk_ad_tile4(int bc, bool react, bool store_rho, int shape, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    if (bc == LB_BC_PERIODIC) ad_tile_bc<LB_BC_PERIODIC>(react, store_rho, shape, st, a, e);
    else ad_tile_bc<LB_BC_OPEN>(react, store_rho, shape, st, a, e);
}

void lbk_ad_step(int bc, bool react, bool store_rho, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    const dim3 block(64, 4), grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4));
    if (bc == LB_BC_PERIODIC) ad_step_go<LB_BC_PERIODIC>(react, store_rho, grid, block, st, a, e);
    else ad_step_go<LB_BC_OPEN>(react, store_rho, grid, block, st, a, e);
}

void lbk_ad_hydro(hipStream_t st, const StepArgs &a) { hipLaunchKernelGGL(k_ad_hydro, cells_grid(a), dim3(256), 0, st, a); }

void lbk_ad_feq(hipStream_t st, const StepArgs &a, float *feq) { hipLaunchKernelGGL(k_ad_feq, cells_grid(a), dim3(256), 0, st, a, feq); }

void lbk_ad_collide(bool react, hipStream_t st, const StepArgs &a, float *f, const float *feq, float G)
{
    if (react) hipLaunchKernelGGL(k_ad_collide<true>, cells_grid(a), dim3(256), 0, st, a, f, feq, G);
    else hipLaunchKernelGGL(k_ad_collide<false>, cells_grid(a), dim3(256), 0, st, a, f, feq, G);
}

void lbk_ad_edge_capture(hipStream_t st, const StepArgs &a, const float *f, float *edge)
{
    const int n = a.fpitch > a.ny ? a.fpitch : a.ny;
    hipLaunchKernelGGL(k_ad_edge_capture, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f, edge);
}

void lbk_ad_edge_patch(hipStream_t st, const StepArgs &a, float *f, const float *edge)
{
    const int n = a.nx > a.ny ? a.nx : a.ny;
    hipLaunchKernelGGL(k_ad_edge_patch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f, edge);
}

long long ad_check_blocks(const StepArgs &a) { return (long long)((a.nx + 255) / 256) * a.ny; }

void lbk_ad_check(hipStream_t st, const StepArgs &a, CheckPartial *part)
{
    hipLaunchKernelGGL(k_ad_check, cells_grid(a), dim3(256), 0, st, a, part);
}
