// scalar_launch.h -- the seam between scalar.cpp, which instantiates the kernels of scalar lattices (kernels_scalar.h), and the host
// units that launch them (launchers.h does the same for the flow kernels).  Arguments are StepArgs as step_args() fills them for the
// handle -- src / dst lattices, rho (stored), u and v (the imposed field: only read), layout, nx, ny, omega -- plus what is below.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"
#include "check_reduce.h"       // CheckPartial

// Edge state of the OPEN family on the device, floats: six rows of fpitch -- south f2, f5, f6, north f4, f7, f8 -- then six columns of
// ny -- west f1, f5, f8, east f3, f6, f7.  (The ABI's order, include/lb_hip.h, is the host's: columns first, rows unpadded.)
struct AdExtra {
    float *edge;        // nullptr in the PERIODIC family
    float G;            // growth rate of the Fisher term; used by the REACT instantiations only
};
inline long long ad_edge_device_floats(long long fpitch, int ny) { return 6 * fpitch + 6LL * ny; }

// bc: LB_BC_PERIODIC or LB_BC_OPEN.  k_ad_step over the whole grid; store_rho: the launch also stores rho.
void lbk_ad_step(int bc, bool react, bool store_rho, hipStream_t st, const StepArgs &a, const AdExtra &e);
// k_ad_tile4: four steps over the whole grid; shape 0: 32 x 16 tiles, two cells per thread; 1: 32 x 16, one; 2: 16 x 16, one
void lbk_ad_tile4(int bc, bool react, bool store_rho, int shape, hipStream_t st, const StepArgs &a, const AdExtra &e);
// the un-fused phases: rho = sum f (a.src); feq from rho, u, v; f (in place) relaxed towards feq
void lbk_ad_hydro(hipStream_t st, const StepArgs &a);
void lbk_ad_feq(hipStream_t st, const StepArgs &a, float *feq);
void lbk_ad_collide(bool react, hipStream_t st, const StepArgs &a, float *f, const float *feq, float G);
// OPEN: the edge state copied out of / written back into the lattice at `f`
void lbk_ad_edge_capture(hipStream_t st, const StepArgs &a, const float *f, float *edge);
void lbk_ad_edge_patch(hipStream_t st, const StepArgs &a, float *f, const float *edge);
// the health check's first pass over the lattice at a.src and the fields a.u, a.v: one record per workgroup, ad_check_blocks(a) of
// them, into part (k_check_final, lb_hip.cpp, folds them)
long long ad_check_blocks(const StepArgs &a);
void lbk_ad_check(hipStream_t st, const StepArgs &a, CheckPartial *part);
