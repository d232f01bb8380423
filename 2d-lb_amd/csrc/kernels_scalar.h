// kernels_scalar.h -- the kernels of scalar lattices (LB_SEM_DIFFUSION: the reference's LB_D2Q9/D2Q9_diffusion.cl, driven as
// reaction_diffusion/diffusion.py:365-380 does: move + copy_buffer -> move_bcs (`pass`) -> update_hydro_diffusion ->
// update_feq_diffusion -> collide_particles[_fisher], five launches and five host waits per step).  Included by scalar.cpp only: its
// plain kernels must be emitted by exactly one translation unit (scalar_launch.h: what the kernels and their host code share; host.h: what the other host units see).
//   k_ad_step<BC, REACT, RHO>   the fused step on the lane-of-four plan (kernels_lane4.h): pull-stream, rho = sum f, linear equilibrium
//                               with the imposed u, v, relaxation [+ growth term]; one 16-byte load each of u and v beside the
//                               gather, rho when asked: 72 B + 8 B per cell and step.  The fused multi-step kernel is held to it bitwise.
//   k_ad_tile4<BC, REACT, RHO, TW, TH, CPT>   four steps per launch in LDS tiles on the plan of k_tile4 (kernels_tile.h), the region's
//                               u, v loaded once for all four; same cell arithmetic (scalar_cell.h): bitwise equal to four k_ad_step
//   k_ad_hydro, k_ad_feq, k_ad_collide<REACT>   the reference's phases one by one (API / test parity; lb_move is k_move + copy).  They
//                               keep the reference's un-fused order -- feq stored, then f (1 - omega) + omega feq -- and so round
//                               differently from the fused cell, where omega enters through rho: held to it by the contract's
//                               tolerance, not bitwise
//   k_ad_step / k_ad_tile4 / k_ad_collide<..., AdNoise>   the noisy instantiations (lb_set_noise; collide_particles_noisy_fisher): an AdNoise
//                               behind the other arguments, the normals drawn in registers from philox.h's stream (scalar_cell.h);
//                               k_ad_tile4<..., AdNoise> bitwise equal to four k_ad_step<..., AdNoise>.  k_ad_noise_fill: lb_noise_fill
//   k_ad_edge_capture / k_ad_edge_patch, k_ad_check (the health check's first pass: check_reduce.h)
// The OPEN family (the reference's box, whose move_bcs does nothing): a link that would enter from outside keeps the value it had
// when the populations were last set -- the handle's edge state, scalar_launch.h.  The gather reads whatever lies beside the box
// (row padding, ghost rows: inside the allocation, never used) and ad_edge_gather puts the edge state in its place.
#pragma once
#include "scalar_cell.h"
#include "scalar_launch.h"
#include "kernels_lane4.h"
#include "kernels_tile.h"       // TileShape, xcd_band_tile

namespace {

// (ad_edge_gather, the OPEN family's edge links of a lane: kernels_lane4.h, shared with kernels_expansion.h)
// moments, equilibrium, relaxation [, growth] of a lane's four gathered cells as two pairs (scalar_cell.h, T = f2a), in place
template <bool REACT>
__device__ __forceinline__ void ad_collide_row(f4a (&q)[9], f4a u4, f4a v4, float omega, float G, f4a &r4)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = pair_of(q[k], h);
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        const f2a rho = ad_rho_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
        ad_relax_t<f2a, REACT>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], omega, G, rho, ux, uy);
        if (h) r4.zw = rho;
        else r4.xy = rho;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) q[k].zw = f[k];
            else q[k].xy = f[k];
        }
    }
}

// The noisy instantiations take an AdNoise behind their other arguments (a pack that is empty or that one struct: the plain
// instantiations keep their signature, their name and their instruction text).
__device__ __forceinline__ const AdNoise &ad_nz(const AdNoise &n) { return n; }

// ... with the noisy collision: ONE Philox call for the lane (box cells x4 .. x4+3 of row y, counter n.t), its four normals in registers
__device__ __forceinline__ void ad_collide_row_noisy(f4a (&q)[9], f4a u4, f4a v4, float omega, float G, const AdNoise &n, int x4, int y,
                                                     f4a &r4)
{
    float z[4];
    ad_lane_normals(n.seed, x4, y, n.t, z);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f2a f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = pair_of(q[k], h);
        const f2a ux = pair_of(u4, h), uy = pair_of(v4, h);
        const f2a rho = ad_rho_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
        ad_relax_noisy_t<f2a>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], omega, G, n.Dg, rho, ux, uy, f2a{z[2 * h], z[2 * h + 1]});
        if (h) r4.zw = rho;
        else r4.xy = rho;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (h) q[k].zw = f[k];
            else q[k].xy = f[k];
        }
    }
}

// (lane_rows and the nine stores written out: through the calls the diagnostic build's OPEN form is scheduled differently, the plane
// offsets are shared with the gather's, and the instruction text moves)
template <int BC, bool REACT, bool RHO, typename... NZ>
__global__ __launch_bounds__(256) void k_ad_step(const StepArgs a, const AdExtra e, const NZ... nz)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= a.fpitch || yl >= a.ny) return;
    int ym = yl - 1, yp = yl + 1;           // source rows of the cy = +1 / cy = -1 links
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a.ny - 1;
        if (yp >= a.ny) yp = 0;
    }
    f4a q[9], r4;
    lane_gather<BC>(a, x4, yl, ym, yp, q);
    if (BC == LB_BC_OPEN) ad_edge_gather(e.edge, a.fpitch, a.nx, a.ny, x4, yl, q);
    const long long m0 = (long long)yl * a.fpitch;
    const f4a u4 = load4<false>(lane_ptr((const float *)a.u + m0, x4));
    const f4a v4 = load4<false>(lane_ptr((const float *)a.v + m0, x4));
    if constexpr (sizeof...(NZ) != 0) ad_collide_row_noisy(q, u4, v4, a.omega, e.G, ad_nz(nz...), x4, yl, r4);
    else ad_collide_row<REACT>(q, u4, v4, a.omega, e.G, r4);
    float *d = a.dst + (long long)yl * a.pitch;
    const long long S = a.plane;
#pragma unroll
    for (int k = 0; k < 9; ++k) store4<false>(lane_ptr(d + k * S, x4), q[k]);
    if (RHO) store4<false>(lane_ptr(a.rho + m0, x4), r4);
}

// The density the populations will have after streaming -- k_ad_step's gather and sum, the same bits -- stored in rho; nothing moves.
// For a velocity that is a function of that density (lb_spectral_velocity, lb_run_screened: spectral.cpp).
template <int BC>
__global__ __launch_bounds__(256) void k_ad_moments(const StepArgs a, const AdExtra e)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yl = blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);
    if (x4 >= a.fpitch || yl >= a.ny) return;
    int ym = yl - 1, yp = yl + 1;
    if (BC == LB_BC_PERIODIC) {
        if (ym < 0) ym = a.ny - 1;
        if (yp >= a.ny) yp = 0;
    }
    f4a q[9], r4;
    lane_gather<BC>(a, x4, yl, ym, yp, q);
    if (BC == LB_BC_OPEN) ad_edge_gather(e.edge, a.fpitch, a.nx, a.ny, x4, yl, q);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f2a rho = ad_rho_t<f2a>(pair_of(q[0], h), pair_of(q[1], h), pair_of(q[2], h), pair_of(q[3], h), pair_of(q[4], h),
                                      pair_of(q[5], h), pair_of(q[6], h), pair_of(q[7], h), pair_of(q[8], h));
        if (h) r4.zw = rho;
        else r4.xy = rho;
    }
    store4<false>(lane_ptr(a.rho + (long long)yl * a.fpitch, x4), r4);
}

// ---- four time steps per launch in LDS tiles -----------------------------------------------------------------------------------------
// k_tile4's plan (kernels_tile.h): a workgroup loads a region -- a TW x TH tile + TILE_T halo cells a side -- of the nine planes AND of
// u, v into LDS once, steps it four times there -- after step s the outermost s rings are stale and no longer computed --, and stores
// the tile (and rho) from the last step; XCD j takes the j-th band of tile rows.  Thread t owns region cells t, t + THREADS, ...
// PERIODIC: a region cell is the image of box cell (gx mod nx, gy mod ny) -- any box, also one smaller than the halo; only the
// un-wrapped tile cells are stored.  OPEN: a region cell outside the box is never stepped (it is loaded from the nearest cell inside,
// so that no address leaves the lattice, and never used); a cell on the box's edge takes its outside links from the edge state, rows
// first, then the columns, as ad_edge_gather does.
// Noisy (an AdNoise or an AdNoiseCell last): step s of the launch draws at counter t + s - 1, in BOX coordinates -- a halo cell and a
// periodic image get the bits their owner gets.  Two plans (DESIGN.md section 17 has both measured):
//   AdNoise      the noise plane: before each step one thread per four region cells (the region's width and origin are multiples of 4:
//                a region four is a box lane-of-four) calls Philox once, as a lane of k_ad_step does, and writes the four normals into
//                an LDS plane beside the populations -- between the two barriers a step has anyway.  A four of a periodic image that is
//                no box lane (nx no multiple of 4, at the seam) falls back to four per-cell draws.
//   AdNoiseCell  every cell calls Philox for the lane of its box coordinates and takes its own word pair (ad_cell_normal): no LDS,
//                four times the integer rounds and twice the transcendental work.  Kept for the A/B measurement.
template <typename... N> struct ad_noise_plan { static constexpr int value = 0; };
template <> struct ad_noise_plan<AdNoise> { static constexpr int value = 1; };
template <> struct ad_noise_plan<AdNoiseCell> { static constexpr int value = 2; };

template <int CELLS>
__device__ __forceinline__ float *ad_noise_plane()
{
    __shared__ float lz[CELLS];
    return lz;
}

template <int BC, int L, int CELLS, int THREADS>
__device__ __forceinline__ void ad_noise_plane_fill(float *lz, const AdNoise &n, unsigned long long t, int gx0, int gy0, int nx, int ny, int tid)
{
    static_assert(L % 4 == 0 && CELLS % 4 == 0, "a region row is whole fours");
    for (int l = tid; l < CELLS / 4; l += THREADS) {
        const int c0 = 4 * l;
        int x = gx0 + c0 % L, y = gy0 + c0 / L;
        if (BC == LB_BC_PERIODIC) {
            x %= nx; if (x < 0) x += nx;
            y %= ny; if (y < 0) y += ny;
            if ((x & 3) != 0 || x + 3 >= nx) {      // not a whole box lane: cell by cell, each wrapped on its own
#pragma unroll 1
                for (int j = 0; j < 4; ++j) lz[c0 + j] = ad_cell_normal(n.seed, (x + j) % nx, y, t);
                continue;
            }
        } else if (x < 0 || x >= nx || y < 0 || y >= ny) {
            continue;                               // outside the box: never stepped
        }
        float z[4];
        ad_lane_normals(n.seed, x, y, t, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) lz[c0 + j] = z[j];
    }
}

template <int BC, bool REACT, bool RHO, int TW, int TH, int CPT, typename... NZ>
__global__ __launch_bounds__((TileShape<TW, TH, CPT>::THREADS)) void k_ad_tile4(const StepArgs a, const AdExtra e, int tiles_x, int n_tiles,
                                                                                const NZ... nz)
{
    constexpr int L = TileShape<TW, TH, CPT>::LW, LH = TileShape<TW, TH, CPT>::LH;
    constexpr int CELLS = TileShape<TW, TH, CPT>::CELLS, THREADS = TileShape<TW, TH, CPT>::THREADS;
    __shared__ float lds[9][CELLS];
    __shared__ float lu[CELLS], lv[CELLS];
    const int tid = threadIdx.x;
    const int tile = a.tile_launch_order ? (int)blockIdx.x : xcd_band_tile(blockIdx.x, n_tiles);
    if (tile >= n_tiles) return;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int gx0 = tx * TW - TILE_T, gy0 = ty * TH - TILE_T;         // global coordinates of region cell (0, 0)
    const long long P = a.pitch, S = a.plane;
    const int nx = a.nx, ny = a.ny;

    int cc[CPT], gxs[CPT], gys[CPT], ring[CPT];
    bool mine[CPT];                                 // mine to store: a cell of the tile, inside the box, not a periodic image
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = tid + i * THREADS;
        const bool have = c < CELLS;
        const int lx = c % L, ly = c / L;
        const int ux = gx0 + lx, uy = gy0 + ly;     // un-wrapped
        int gx = ux, gy = uy;
        bool inside = true;
        if (BC == LB_BC_PERIODIC) {
            gx %= nx; if (gx < 0) gx += nx;
            gy %= ny; if (gy < 0) gy += ny;
        } else {
            inside = ux >= 0 && ux < nx && uy >= 0 && uy < ny;
            gx = min(max(ux, 0), nx - 1);
            gy = min(max(uy, 0), ny - 1);
        }
        cc[i] = c; gxs[i] = gx; gys[i] = gy;
        ring[i] = (have && inside) ? min(min(lx, L - 1 - lx), min(ly, LH - 1 - ly)) : -1;
        mine[i] = ux >= 0 && ux < nx && uy >= 0 && uy < ny;
        if (have) {
            const long long o = (long long)gy * P + gx, m = (long long)gy * a.fpitch + gx;
#pragma unroll
            for (int k = 0; k < 9; ++k) lds[k][c] = a.src[k * S + o];
            lu[c] = a.u[m];
            lv[c] = a.v[m];
        }
    }
    constexpr int NOISE_PLAN = ad_noise_plan<NZ...>::value;
    float *lz = nullptr;
    if constexpr (NOISE_PLAN == 1) {
        lz = ad_noise_plane<CELLS>();
        ad_noise_plane_fill<BC, L, CELLS, THREADS>(lz, ad_nz(nz...), ad_nz(nz...).t, gx0, gy0, nx, ny, tid);
    }
    __syncthreads();

#pragma unroll 1
    for (int s = 1; s <= TILE_T; ++s) {
        const bool last = (s == TILE_T);
        float q[CPT][9];
        bool act[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            act[i] = ring[i] >= s;
            if (!act[i]) continue;
            const int c = cc[i], gx = gxs[i], gy = gys[i];
            float f0 = lds[0][c], f1 = lds[1][c - 1], f2 = lds[2][c - L], f3 = lds[3][c + 1], f4 = lds[4][c + L];
            float f5 = lds[5][c - L - 1], f6 = lds[6][c - L + 1], f7 = lds[7][c + L + 1], f8 = lds[8][c + L - 1];
            if (BC == LB_BC_OPEN && (gx == 0 || gx == nx - 1 || gy == 0 || gy == ny - 1)) {
                const float *row = e.edge + gx, *col = e.edge + 6LL * a.fpitch + gy;
                if (gy == 0) { f2 = row[0]; f5 = row[a.fpitch]; f6 = row[2 * a.fpitch]; }
                if (gy == ny - 1) { f4 = row[3 * a.fpitch]; f7 = row[4 * a.fpitch]; f8 = row[5 * a.fpitch]; }
                if (gx == 0) { f1 = col[0]; f5 = col[ny]; f8 = col[2 * ny]; }
                if (gx == nx - 1) { f3 = col[3 * ny]; f6 = col[4 * ny]; f7 = col[5 * ny]; }
            }
            const float rho = ad_rho_t<float>(f0, f1, f2, f3, f4, f5, f6, f7, f8);
            if constexpr (sizeof...(NZ) != 0) {
                const AdNoise &n = ad_nz(nz...);
                float z;
                if constexpr (NOISE_PLAN == 1) z = lz[c];
                else z = ad_cell_normal(n.seed, gx, gy, n.t + (unsigned long long)(s - 1));
                ad_relax_noisy_t<float>(f0, f1, f2, f3, f4, f5, f6, f7, f8, a.omega, e.G, n.Dg, rho, lu[c], lv[c], z);
            } else {
                ad_relax_t<float, REACT>(f0, f1, f2, f3, f4, f5, f6, f7, f8, a.omega, e.G, rho, lu[c], lv[c]);
            }
            if (last) {
                if (mine[i]) {
                    float *d = a.dst + (long long)gy * P + gx;
                    d[0] = f0; d[S] = f1; d[2 * S] = f2; d[3 * S] = f3; d[4 * S] = f4;
                    d[5 * S] = f5; d[6 * S] = f6; d[7 * S] = f7; d[8 * S] = f8;
                    if (RHO) a.rho[(long long)gy * a.fpitch + gx] = rho;
                }
            } else {
                q[i][0] = f0; q[i][1] = f1; q[i][2] = f2; q[i][3] = f3; q[i][4] = f4;
                q[i][5] = f5; q[i][6] = f6; q[i][7] = f7; q[i][8] = f8;
            }
        }
        if (last) break;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CPT; ++i)
            if (act[i]) {
#pragma unroll
                for (int k = 0; k < 9; ++k) lds[k][cc[i]] = q[i][k];
            }
        if constexpr (NOISE_PLAN == 1)              // the next step's normals (everyone has read this step's: the barrier above)
            ad_noise_plane_fill<BC, L, CELLS, THREADS>(lz, ad_nz(nz...), ad_nz(nz...).t + (unsigned long long)s, gx0, gy0, nx, ny, tid);
        __syncthreads();
    }
}

// ---- the reference's phases, one cell per thread: grid = (ceil(nx / 256), ny) ---------------------------------------------------
__global__ void k_ad_hydro(const StepArgs a)                    // D2Q9_diffusion.cl:41-68: rho only; u, v are imposed
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const float *f = a.src + (long long)y * a.pitch + x;
    const long long S = a.plane;
    a.rho[(long long)y * a.fpitch + x] = ad_rho_t<float>(f[0], f[S], f[2 * S], f[3 * S], f[4 * S], f[5 * S], f[6 * S], f[7 * S], f[8 * S]);
}

__global__ void k_ad_feq(const StepArgs a, float *feq)         // :1-38
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long m = (long long)y * a.fpitch + x;
    float e[9];
    ad_feq_cell(e, a.rho[m], a.u[m], a.v[m]);
    float *o = feq + (long long)y * a.pitch + x;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k * a.plane] = e[k];
}

// Noisy (an AdNoise last; :127-167): z from the supplied field where there is one (lb_set_noise_field), else from the stream
template <bool REACT, typename... NZ>
__global__ void k_ad_collide(const StepArgs a, float *f, const float *feq, float G, const NZ... nz)     // :70-93, :95-124
{
    int x, y;
    if (!cell_xy(a, x, y)) return;
    const long long o = (long long)y * a.pitch + x;
    const float keep = 1.f - a.omega;
    float react = 0.f;
    if constexpr (sizeof...(NZ) != 0) {
        const AdNoise &n = ad_nz(nz...);
        const float z = n.field ? n.field[(long long)y * a.nx + x] : ad_cell_normal(n.seed, x, y, n.t);
        react = ad_noisy_react_t<float>(G, n.Dg, a.rho[(long long)y * a.fpitch + x], z);
    } else if (REACT) {
        const float rho = a.rho[(long long)y * a.fpitch + x];
        react = (G * rho) * (1.f - rho);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float v = lb_fma(f[o + k * a.plane], keep, a.omega * feq[o + k * a.plane]);
        if (REACT) v = lb_fma(lb_w9(k), react, v);
        if constexpr (sizeof...(NZ) != 0) v = ad_clamp0(v);
        f[o + k * a.plane] = v;
    }
}

// lb_noise_fill: the normals of noise counter n.t as dense [ny][nx] floats, one lane-of-four per thread as k_ad_step draws them;
// grid = (ceil(nx / 1024), ny), 256 threads
__global__ __launch_bounds__(256) void k_ad_noise_fill(const AdNoise n, int nx, float *out)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= nx) return;
    float z[4];
    ad_lane_normals(n.seed, x4, y, n.t, z);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x4 + j < nx) out[(long long)y * nx + x4 + j] = z[j];
}

// ---- OPEN: edge state <-> lattice.  One thread per column / row index: grid = ceil(max(fpitch, ny) / 256) --------------------------
__device__ __constant__ int ad_row_k[6] = {2, 5, 6, 4, 7, 8};       // south f2, f5, f6; north f4, f7, f8
__device__ __constant__ int ad_col_k[6] = {1, 5, 8, 3, 6, 7};       // west f1, f5, f8; east f3, f6, f7

__global__ void k_ad_edge_capture(const StepArgs a, const float *f, float *edge)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.fpitch)
        for (int r = 0; r < 6; ++r) {
            const int y = r < 3 ? 0 : a.ny - 1;
            edge[(long long)r * a.fpitch + i] = i < a.nx ? f[ad_row_k[r] * a.plane + (long long)y * a.pitch + i] : 0.f;
        }
    if (i < a.ny)
        for (int c = 0; c < 6; ++c) {
            const int x = c < 3 ? 0 : a.nx - 1;
            edge[6LL * a.fpitch + (long long)c * a.ny + i] = f[ad_col_k[c] * a.plane + (long long)i * a.pitch + x];
        }
}

__global__ void k_ad_edge_patch(const StepArgs a, float *f, const float *edge)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nx)
        for (int r = 0; r < 6; ++r) {
            // (the four corner links that belong to a column as well are the column's: f5(0,0), f6(nx-1,0), f8(0,ny-1), f7(nx-1,ny-1))
            if ((i == 0 && (r == 1 || r == 5)) || (i == a.nx - 1 && (r == 2 || r == 4))) continue;
            const int y = r < 3 ? 0 : a.ny - 1;
            f[ad_row_k[r] * a.plane + (long long)y * a.pitch + i] = edge[(long long)r * a.fpitch + i];
        }
    if (i < a.ny)
        for (int c = 0; c < 6; ++c) {
            const int x = c < 3 ? 0 : a.nx - 1;
            f[ad_col_k[c] * a.plane + (long long)i * a.pitch + x] = edge[6LL * a.fpitch + (long long)c * a.ny + i];
        }
}

// ---- health check: non-finite cells, sum of rho = sum of the populations, max |u|^2 of the imposed field ------------------------------
// grid = (ceil(nx / 256), ny), 256 threads, one partial per workgroup (check_reduce.h); k_check_final (kernels_check.h) folds them
__global__ __launch_bounds__(256) void k_ad_check(const StepArgs a, CheckPartial *part)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    double s = 0.0;
    unsigned long long n = 0;
    float m = 0.f;
    if (x < a.nx) {
        const float *f = a.src + (long long)y * a.pitch + x;
        const long long S = a.plane, o = (long long)y * a.fpitch + x;
        const float rho = ad_rho_t<float>(f[0], f[S], f[2 * S], f[3 * S], f[4 * S], f[5 * S], f[6 * S], f[7 * S], f[8 * S]);
        const float ux = a.u[o], uy = a.v[o], usq = ux * ux + uy * uy;
        if (fabsf(rho) <= 3.0e38f && fabsf(usq) <= 3.0e38f) { s = (double)rho; m = usq; }     // (false for NaN)
        else n = 1;
    }
    check_reduce_block<4>(s, n, m, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}

}  // namespace
