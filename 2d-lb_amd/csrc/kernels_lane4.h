// kernels_lane4.h -- the lane-of-four plan of every handle kind beyond flow, once.  Included after kernels_fused.h by the kind kernel
// headers (kernels_scalar.h, kernels_multifield.h, kernels_poisson.h, kernels_porous.h, kernels_multifluid.h, kernels_rocket.h) and by
// kernels_nutrient.h and kernels_expansion.h, the sets of scalar lattices that are no kind.  Device
// functions only: no kernel is emitted from here.
// The plan: a lane owns four consecutive cells (x4 .. x4+3) of one row and a wave 256 cells of it; launch blockDim = (64, 4), grid =
// (ceil(fpitch / 256), ceil(ny / 4)).  The source rows are wrapped or clamped as the boundary family says (lane_rows), the nine planes
// are gathered by k_step's gather -- nine 16-byte loads, six displaced by one element -- (lane_gather), the four cells are collided
// as two pairs of x-adjacent cells (T = f2a; pair_of), and nine aligned 16-byte stores follow (store_planes): 72 B per cell, lattice
// and step.  The families: LB_BC_PERIODIC wraps; LB_BC_ZERO_GRADIENT clamps the SOURCE cell to [1, n-2] (kernels_porous.h has why);
// every other one gathers without a wrap -- it reads row padding and ghost rows beside the box, inside the allocation -- and the kind
// replaces what entered from outside.
// A step that is not local to the cell reads a density around the lane's cells: from memory (lane_nb_load) or, in the one-launch form,
// from the LDS rows of a workgroup that owns R rows of a 256-cell tile (LANE4_LDS_ROW; cell_rho for the halo columns).
// Behind them what the un-fused phases share: one cell per thread (cell_xy, load_cell, lb_w9), a closed box's wall rule on a lane's
// row (row_wall) and the walk along a box's edge (edge_walk, BoxEdge).
// Every kernel built on these holds the instruction text it had with the code written out (tools/isa_diff.py).  A helper is optimised
// on its own before it is inlined, so a call can order or share arithmetic differently from the same statements in the kernel: where it
// did, the kernel keeps them written out and says so at the place.
#pragma once
#include "kernels_fused.h"

namespace {

// pair h of a lane's four values: the cells x4, x4+1 or x4+2, x4+3
__device__ __forceinline__ f2a pair_of(f4a v, int h) { return h ? v.zw : v.xy; }

__device__ __forceinline__ f4a sum9(const f4a (&q)[9]) { return q[0] + q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7] + q[8]; }

// The lane's cells and rows: x4, yl (wave-uniform), ys the row of the source cells, ym / yp the source rows of the cy = +1 / cy = -1
// links.  False: nothing of the lane is in the lattice (x4, yl are set all the same).
template <int BC>
__device__ __forceinline__ bool lane_rows(const StepArgs &a, int &x4, int &yl, int &ys, int &ym, int &yp)
{
    x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= a.fpitch || yl >= a.ny) return false;
    ys = yl;
    if (BC == LB_BC_ZERO_GRADIENT) ys = min(max(yl, 1), a.ny - 2);
    ym = ys - 1, yp = ys + 1;
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a.ny - 1;
        if (yp >= a.ny) yp = 0;
    }
    return true;
}

// ZERO_GRADIENT, x: the lane's cells x = 0 and x = nx-1 become copies of their interior neighbours (ys: the clamped row): a select
// where the neighbour is in the lane, nine scalar loads on that one lane where nx-1 is a lane's first cell
__device__ __forceinline__ void clamp_x(const StepArgs &a, int x4, int ys, f4a (&q)[9])
{
    if (x4 == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k].x = q[k].y;
    }
    const int c = a.nx - 1 - x4;
    if (c == 0) {
        // the neighbour is the last cell of the lane before: gathered again, link k from (nx-2 - c_kx, ys - c_ky)
        const long long P = a.pitch, S = a.plane;
        const float *r0 = a.src + (long long)ys * P + (a.nx - 2), *rm = r0 - P, *rp = r0 + P;
        q[0].x = r0[0];
        q[1].x = r0[1 * S - 1];
        q[2].x = rm[2 * S];
        q[3].x = r0[3 * S + 1];
        q[4].x = rp[4 * S];
        q[5].x = rm[5 * S - 1];
        q[6].x = rm[6 * S + 1];
        q[7].x = rp[7 * S + 1];
        q[8].x = rp[8 * S - 1];
    } else if (c > 0 && c < 4) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 1; j < 4; ++j) q[k][j] = j == c ? q[k][j - 1] : q[k][j];
    }
}

// k_step's gather (its PIPE form is the one without a wrap in x) and, for ZERO_GRADIENT, the clamp in x -- unless the caller puts
// clamp_x somewhere behind the gather itself (CLAMP_X = false)
template <int BC, bool CLAMP_X = true>
__device__ __forceinline__ void lane_gather(const StepArgs &a, int x4, int ys, int ym, int yp, f4a (&q)[9])
{
    uc4 mk;
    gather_row<BC == LB_BC_PERIODIC ? LB_BC_PERIODIC : LB_BC_PIPE, false, false>(a, x4, ys, ym, yp, q, mk);
    if (CLAMP_X && BC == LB_BC_ZERO_GRADIENT) clamp_x(a, x4, ys, q);
}

// the nine aligned 16-byte stores of a lane's four cells of row yl
__device__ __forceinline__ void store_planes(const StepArgs &a, int yl, int x4, const f4a (&q)[9])
{
    float *d = a.dst + (long long)yl * a.pitch;
    const long long S = a.plane;
#pragma unroll
    for (int k = 0; k < 9; ++k) store4<false>(lane_ptr(d + k * S, x4), q[k]);
}

// The scalar lattice's OPEN family (kernels_scalar.h, kernels_expansion.h): the links of a lane's four cells (x4 .. x4+3, row y) that enter from outside the box, from the edge state.  The column's
// entry goes in last: it is the one that counts where a corner link belongs to a row as well.
__device__ __forceinline__ void ad_edge_gather(const float *edge, int fpitch, int nx, int ny, int x4, int y, f4a (&q)[9])
{
    if (y == 0) {
        q[2] = load4<false>(lane_ptr(edge, x4));
        q[5] = load4<false>(lane_ptr(edge + fpitch, x4));
        q[6] = load4<false>(lane_ptr(edge + 2 * fpitch, x4));
    }
    if (y == ny - 1) {
        q[4] = load4<false>(lane_ptr(edge + 3 * fpitch, x4));
        q[7] = load4<false>(lane_ptr(edge + 4 * fpitch, x4));
        q[8] = load4<false>(lane_ptr(edge + 5 * fpitch, x4));
    }
    const float *col = edge + 6LL * fpitch + y;
    if (x4 == 0) {
        q[1].x = col[0];
        q[5].x = col[ny];
        q[8].x = col[2 * ny];
    }
    const int c = nx - 1 - x4;
    if (c >= 0 && c < 4) {
        const float e3 = col[3 * ny], e6 = col[4 * ny], e7 = col[5 * ny];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            q[3][j] = j == c ? e3 : q[3][j];
            q[6][j] = j == c ? e6 : q[6][j];
            q[7][j] = j == c ? e7 : q[7][j];
        }
    }
}

// ---- a density around a lane's four cells -----------------------------------------------------------------------------------------
// nb[row][col], row 0 = yl - 1, col 0 = x4 - 1 ... col 5 = x4 + 4: one 16-byte load and two 4-byte loads per row.  Every index is
// inside the box -- wrapped (PERIODIC) or clamped to [0, n-1]: the neighbour outside is the edge cell itself --, so nothing outside
// the row's allocation is read; cells past nx-1 (row padding) get in-bounds values nobody uses.
template <int BC>
__device__ __forceinline__ void lane_nb_load(const float *rho, int fpitch, int nx, int ny, int x4, int yl, float (&nb)[3][6])
{
    const int c = nx - 1 - x4;
    int xl = x4 - 1, xr = x4 + 4;
    if (xl < 0) xl = BC == LB_BC_PERIODIC ? nx - 1 : 0;
    if (xr >= nx) xr = BC == LB_BC_PERIODIC ? 0 : nx - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        int y = yl - 1 + r;
        if (BC == LB_BC_PERIODIC) {
            if (y < 0) y = ny - 1;
            if (y >= ny) y = 0;
        } else {
            y = min(max(y, 0), ny - 1);
        }
        const float *row = rho + (long long)y * fpitch;
        const f4a v = load4<false>(lane_ptr(row, x4));
        const float w = row[xl], e = row[xr];
        nb[r][0] = w;
        nb[r][1] = v.x;
        // the east neighbour of the cell nx-1, where that cell is not the lane's last: the wrapped cell / the cell itself
        nb[r][2] = c == 0 ? (BC == LB_BC_PERIODIC ? e : v.x) : v.y;
        nb[r][3] = c == 1 ? (BC == LB_BC_PERIODIC ? e : v.y) : v.z;
        nb[r][4] = c == 2 ? (BC == LB_BC_PERIODIC ? e : v.z) : v.w;
        nb[r][5] = e;
    }
}

// the density of the cell (x, row) as lane_gather and sum9 compute it, by nine 4-byte loads: ys, ym, yp as lane_rows gives them
template <int BC>
__device__ __forceinline__ float cell_rho(const StepArgs &a, int x, int ys, int ym, int yp)
{
    int xs = x;
    if (BC == LB_BC_ZERO_GRADIENT) xs = min(max(x, 1), a.nx - 2);
    int xm = xs - 1, xp = xs + 1;           // source columns of the cx = +1 / cx = -1 links
    if (BC == LB_BC_PERIODIC) {
        if (xm < 0) xm = a.nx - 1;
        if (xp >= a.nx) xp = 0;
    }
    const long long P = a.pitch, S = a.plane;
    const float *r0 = a.src + (long long)ys * P, *rm = a.src + (long long)ym * P, *rp = a.src + (long long)yp * P;
    const float f0 = r0[xs], f1 = r0[1 * S + xm], f2 = rm[2 * S + xs], f3 = r0[3 * S + xp], f4 = rp[4 * S + xs];
    const float f5 = rm[5 * S + xm], f6 = rm[6 * S + xp], f7 = rp[7 * S + xp], f8 = rp[8 * S + xm];
    return f0 + f1 + f2 + f3 + f4 + f5 + f6 + f7 + f8;
}

// ---- the one-launch form of such a step -------------------------------------------------------------------------------------------
// Launch: blockDim = (64, R + 2), grid = (ceil(fpitch / 256), ceil(ny / R)).  A workgroup owns R rows of a 256-cell tile.  Wave w
// gathers the populations of row y0 - 1 + w (the rows above and below the owned ones wrapped or clamped into the box: the halo rows)
// and puts the density of its 256 cells into its LDS row, lane 0 and lane 1 also that of the cell west of the tile and of the cell east
// of its last cell in the box (wrapped, or the edge cell itself: the halo columns, cell_rho).  After ONE barrier the waves of the owned
// rows, whose populations stayed in registers, read the density around their cells from LDS (lane_nb_load's layout); the halo waves
// are done.  An LDS row: LANE4_LDS_ROW floats, cell x of the tile at index 4 + x (16-byte aligned), the west halo at 3, the east halo at
// 4 + (cells of the tile inside the box).  k_mc_step and k_ry_step each write the index arithmetic out; so does k_sn_step, whose LDS rows hold an
// operand of a STORED plane: its halo rows are read by the owned rows' waves, no wave gathers for them.
constexpr int LANE4_LDS_ROW = 264;

// ---- the reference's phases, one cell per thread: grid = (ceil(nx / 256), ny) -------------------------------------------------------
__device__ __forceinline__ bool cell_xy(const StepArgs &a, int &x, int &y)
{
    x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    return x < a.nx;
}

__device__ __forceinline__ void load_cell(const float *p, long long S, float (&f)[9])
{
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = p[k * S];
}

// the lattice weight of link k (k a constant once the loop over the links is unrolled)
__device__ __forceinline__ float lb_w9(int k)
{
    const float w[9] = {4.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 9.f, 1.f / 36.f, 1.f / 36.f, 1.f / 36.f, 1.f / 36.f};
    return w[k];
}

// ---- closed boxes: a cell rule on the walls ---------------------------------------------------------------------------------------
// A cell rule is a struct passed by value whose rule(c, w, e, s, n, st) rewrites the links of one cell that entered from outside
// (w, e, s, n: it lies in column 0 / nx-1, row 0 / ny-1; st: the eight corner links in the ABI's order -- f6, f8 of (0,0), f5, f7 of
// (nx-1,0), f5, f7 of (0,ny-1), f6, f8 of (nx-1,ny-1)): MfBox (kernels_multifield.h), PsBox (kernels_poisson.h).
// ... on a lane's four gathered cells (x4 .. x4+3, row y); st: the lattice's corner state.  The caller has checked that the lane holds
// a wall cell.
template <typename Rule>
__device__ __forceinline__ void row_wall(Rule rule, const float *st, int nx, int ny, int x4, int y, f4a (&q)[9])
{
    const bool s = (y == 0), n = (y == ny - 1);
    const int ce = nx - 1 - x4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool w = (x4 == 0 && j == 0), e = (j == ce);
        if (s || n || w || e) {
            Cell c = row_cell(q, j);
            rule.rule(c, w, e, s, n, st);
            row_cell_put(q, j, c);
        }
    }
}

// ... as an edge rule (edge_walk): the cell (x, y) of lattice f in place.  The two links per corner that are neither streamed nor
// written are what the lattice holds (lb_move has patched the corner state in).
template <typename Rule>
struct BoxEdge {
    Rule r;
    __device__ __forceinline__ void edge_cell(const StepArgs &a, float *f, int x, int y) const
    {
        float *p = f + (long long)y * a.pitch + x;
        const long long S = a.plane;
        Cell c = {p[0], p[S], p[2 * S], p[3 * S], p[4 * S], p[5 * S], p[6 * S], p[7 * S], p[8 * S]};
        const float own[8] = {c.f6, c.f8, c.f5, c.f7, c.f5, c.f7, c.f6, c.f8};
        r.rule(c, x == 0, x == a.nx - 1, y == 0, y == a.ny - 1, own);
        p[S] = c.f1; p[2 * S] = c.f2; p[3 * S] = c.f3; p[4 * S] = c.f4;
        p[5 * S] = c.f5; p[6 * S] = c.f6; p[7 * S] = c.f7; p[8 * S] = c.f8;
    }
};

// The un-fused boundary pass of a box, in place behind lb_move: one thread per index i, grid = ceil(max(nx, ny) / 256): the cells
// (i, 0) and (i, ny-1) of the edge rows, (0, i) and (nx-1, i) of the edge columns between them.
template <typename Edge>
__device__ __forceinline__ void edge_walk(const StepArgs &a, float *f, Edge edge)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nx) {
        edge.edge_cell(a, f, i, 0);
        edge.edge_cell(a, f, i, a.ny - 1);
    }
    if (i >= 1 && i <= a.ny - 2) {
        edge.edge_cell(a, f, 0, i);
        edge.edge_cell(a, f, a.nx - 1, i);
    }
}

}  // namespace
