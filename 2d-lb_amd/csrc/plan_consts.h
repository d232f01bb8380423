// plan_consts.h -- the few numbers the kernels and the launch planner (plan.h) must agree on; the bits of the variant word are the
// public header's (lb_variant_bits).
// Plain C++: the kernel headers include it for their own use, plan.cpp includes nothing of HIP.  One definition each; why a number
// has its value is told beside the kernel that uses it.
#pragma once

// LB_VAR_* (the automatic choice: effective_variant, plan.cpp)
#include "../../include/lb_hip.h"

namespace {

constexpr int GHOST = 14;  // ghost rows below row 0 and above row H-1 of every plane: a slab runs two seven-step
                           // launches per halo exchange, the first one recomputing 7 of the neighbour's rows
constexpr int MAX_DEPTH = 7;            // deepest fused kernel

// Template value of the PIPE family run with the kernels of the reference's D2Q9i.cl fork (lb_params.semantics =
// LB_SEM_OPENCL_D2Q9I); not a public lb_bc_mode.
constexpr int LB_BC_PIPE_I = 4;

constexpr int STRIP_W = 256;       // cells per wave-row (kernels_fused.h)

constexpr int STEP4_WAVES = 2;      // waves per workgroup = the two directions of a segment pair: 2 x 2 windows x 9 KiB of LDS (kernels_step4.h)

// (kernels_step5.h: why the strips lie 240 and not 248 cells apart)
constexpr int STEP5_SKIRT = 8;                          // cells a strip starts before / ends behind its stored cells (= one lane)
constexpr int STEP5_VALID = STRIP_W - 2 * STEP5_SKIRT;  // 248 cells stored per strip and row
// strips a grid of nx columns is cut into
constexpr int step5_strips(int nx) { return (nx + STEP5_VALID - 1) / STEP5_VALID; }

// (kernels_deep.h) The skirt is D - 1 cells deep, i.e. whole lanes of four cells that are computed and never stored, at either end of a strip
constexpr int deep_skirt_lanes(int D) { return (D - 1 + 3) / 4; }
constexpr int deep_valid(int D) { return STRIP_W - 8 * deep_skirt_lanes(D); }           // cells stored per strip and row (D = 6..9: 240)
constexpr int deep_strips(int nx, int D) { return (nx + deep_valid(D) - 1) / deep_valid(D); }

constexpr int TILE_T = 4;                   // time steps per pass of the LDS tiles = halo width (kernels_tile.h)

constexpr int RY_ROWS = 10;                 // rows of a 256-cell tile a workgroup of k_ry_step owns (kernels_rocket.h, rocket.cpp)

}  // namespace
