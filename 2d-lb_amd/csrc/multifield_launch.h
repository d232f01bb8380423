// multifield_launch.h -- the seam between multifield.cpp, which instantiates the kernels of coupled scalar lattices
// (kernels_multifield.h: LB_SEM_MULTIFIELD), and the host unit that launches them (scalar_launch.h does the same for lattices on their own).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_fused.h"      // StepArgs

// The fields of a coupled set advanced by one launch: StepArgs as step_args() fills them for each member (a[i].omega its omega,
// a[i].corner its corner state: the eight never-written corner links of LB_BC_BOX in the ABI's order, include/lb_hip.h), its
// growth rate and -- lbk_mf_collide only -- its feq lattice.  The imposed velocity every field reads is a[0].u, a[0].v.
constexpr int MF_MAX = 4;
struct MfArgs {
    StepArgs a[MF_MAX];
    float G[MF_MAX];
    const float *feq[MF_MAX];
};

// bc: LB_BC_PERIODIC or LB_BC_BOX; nf = 1 ... MF_MAX.  k_mf_step over the whole grid; store_rho: the launch also stores every field's rho.
void lbk_mf_step(int bc, int nf, bool store_rho, hipStream_t st, const MfArgs &m);
// LB_BC_BOX: the in-place bounce-back of move_bcs on the lattice at f (edge cells only)
void lbk_mf_move_bcs(hipStream_t st, const StepArgs &a, float *f);
// the un-fused collide_particles of the set: a[i].src relaxed in place towards feq[i], growth from the stored a[i].rho
void lbk_mf_collide(int nf, hipStream_t st, const MfArgs &m);
