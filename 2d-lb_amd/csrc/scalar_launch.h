// scalar_launch.h -- what the kernels of scalar lattices (kernels_scalar.h) and the host code that launches them (scalar.cpp) share
// beyond StepArgs.  Arguments are StepArgs as step_args() fills them for the handle -- src / dst lattices, rho (stored), u and v (the
// imposed field: only read), layout, nx, ny, omega -- plus what is below.
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
// The noisy collision (lb_set_noise; philox.h has the stream): taken, behind AdExtra, by the noisy instantiations only.
struct AdNoise {
    float Dg;                   // the noise strength: react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z
    unsigned long long seed;    // the key
    unsigned long long t;       // the noise counter of the launch's first collision
    const float *field;         // the un-fused collision only: a supplied [ny][nx] field of normals in place of the stream, or nullptr
};
struct AdNoiseCell : AdNoise {};     // k_ad_tile4 only: the per-cell plan instead of the noise plane (kernels_scalar.h)
inline long long ad_edge_device_floats(long long fpitch, int ny) { return 6 * fpitch + 6LL * ny; }
