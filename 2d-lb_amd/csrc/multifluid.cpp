// multifluid.cpp -- the translation unit of multicomponent Shan-Chen fluids: instantiates and launches the kernels of
// kernels_multifluid.h (multifluid_launch.h).
#include "kernels_multifluid.h"

namespace {

dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }
dim3 step_grid(const StepArgs &a) { return dim3((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4)); }

template <int BC, int NF>
void launch_moments(hipStream_t st, const McArgs &m)
{
    hipLaunchKernelGGL((k_mc_moments<BC, NF>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

template <int BC, int NF>
void launch_collide(bool last, hipStream_t st, const McArgs &m)
{
    if (last) hipLaunchKernelGGL((k_mc_collide<BC, NF, true>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
    else hipLaunchKernelGGL((k_mc_collide<BC, NF, false>), step_grid(m.a[0]), dim3(64, 4), 0, st, m);
}

// rows a workgroup of k_mc_step owns: six (eight waves, two per SIMD: at most 256 registers each) for one and two fluids; two (four
// waves, one per SIMD) for three, whose cell does not fit 256 registers (tools/kernel_resources.py multifluid.cpp k_mc)
template <int NF>
constexpr int step_rows() { return NF == 3 ? 2 : 6; }

template <int BC, int NF>
void launch_step(bool last, hipStream_t st, const McArgs &m)
{
    constexpr int R = step_rows<NF>();
    const StepArgs &a = m.a[0];
    const dim3 grid((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + R - 1) / R)), block(64, R + 2);
    if (last) hipLaunchKernelGGL((k_mc_step<BC, NF, R, true>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((k_mc_step<BC, NF, R, false>), grid, block, 0, st, m);
}

template <int BC, int NF>
void launch_forces(hipStream_t st, const McArgs &m)
{
    hipLaunchKernelGGL((k_mc_forces<BC, NF>), cells_grid(m.a[0]), dim3(256), 0, st, m);
}

// f<BC, NF>(args...) for the run-time bc and nf
#define MC_DISPATCH(f, ...)                                                 \
    do {                                                                    \
        if (bc == LB_BC_PERIODIC) {                                         \
            if (nf == 1) f<LB_BC_PERIODIC, 1>(__VA_ARGS__);                 \
            else if (nf == 2) f<LB_BC_PERIODIC, 2>(__VA_ARGS__);            \
            else f<LB_BC_PERIODIC, 3>(__VA_ARGS__);                         \
        } else {                                                            \
            if (nf == 1) f<LB_BC_ZERO_GRADIENT, 1>(__VA_ARGS__);            \
            else if (nf == 2) f<LB_BC_ZERO_GRADIENT, 2>(__VA_ARGS__);       \
            else f<LB_BC_ZERO_GRADIENT, 3>(__VA_ARGS__);                    \
        }                                                                   \
    } while (0)

}  // namespace

void lbk_mc_moments(int bc, int nf, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_moments, st, m); }

void lbk_mc_collide(int bc, int nf, bool last, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_collide, last, st, m); }

void lbk_mc_step(int bc, int nf, bool last, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_step, last, st, m); }

void lbk_mc_forces(int bc, int nf, hipStream_t st, const McArgs &m) { MC_DISPATCH(launch_forces, st, m); }

void lbk_mc_hydro(hipStream_t st, const StepArgs &a) { hipLaunchKernelGGL(k_mc_hydro, cells_grid(a), dim3(256), 0, st, a); }

void lbk_mc_bary(int nf, hipStream_t st, const McArgs &m)
{
    const dim3 grid = cells_grid(m.a[0]);
    if (nf == 1) hipLaunchKernelGGL(k_mc_bary<1>, grid, dim3(256), 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mc_bary<2>, grid, dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_mc_bary<3>, grid, dim3(256), 0, st, m);
}

void lbk_mc_relax(hipStream_t st, const StepArgs &a, const PmExtra &e, float *f, const float *feq)
{
    hipLaunchKernelGGL(k_mc_relax, cells_grid(a), dim3(256), 0, st, a, e, f, feq);
}

void lbk_mc_react(int nf, hipStream_t st, const McArgs &m)
{
    const dim3 grid = cells_grid(m.a[0]);
    if (nf == 1) hipLaunchKernelGGL(k_mc_react<1>, grid, dim3(256), 0, st, m);
    else if (nf == 2) hipLaunchKernelGGL(k_mc_react<2>, grid, dim3(256), 0, st, m);
    else hipLaunchKernelGGL(k_mc_react<3>, grid, dim3(256), 0, st, m);
}
