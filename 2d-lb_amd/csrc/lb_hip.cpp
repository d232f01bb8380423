// lb_hip.cpp -- MI355X (gfx950 / CDNA4) D2Q9 BGK lattice-Boltzmann engine behind the C ABI
// of include/lb_hip.h.  Written for gfx950 only: wave64, 16-byte-per-lane global accesses,
// one fused pull kernel per time step (72 algorithmic bytes per lattice update), no MFMA
// (the path is a memory-bound stencil).
//
// What it replaces (reference = latticeboltzmann/2d-lb):
//   LB_D2Q9/D2Q9.cl               update_feq :2-64, update_hydro :67-100, collide_particles :102-121,
//                                 copy_buffer :123-137, move :139-171, move_bcs :173-261,
//                                 set_zero_velocity_in_obstacle :377-396, bounceback_in_obstacle :398-433
//   LB_D2Q9/dimensionless/opencl_dim.py   the pyopencl buffer/queue plumbing (:203-255, 291-293,
//                                 323-327, 395-407) and the per-step launch sequence of run() (:372-387)
//
// Device layout: structure of arrays, nine planes per lattice, two lattices (A/B).  A plane-row
// is `pitch` floats (nx rounded up to 64 floats = 256 B); the nine plane-rows of one lattice row are stored together
// ([row][plane][pitch]: the marching kernels then stream 2 regions per segment instead of 18 -- +12 % at 8192^2,
// profiles/r02_experiments.txt; LB_FLAG_PLANAR keeps each plane contiguous, [plane][row][pitch]).  Rows -GHOST..-1 and
// H..H+GHOST-1 are ghost rows (GHOST = 14: slab halo, deep enough for two seven-step launches per exchange / don't-care
// at walls), so element (k, x, y) of a slab of H rows lives at
//   lattice + GUARD + (y+GHOST)*rowp + k*plane + x,      rowp = 9*pitch, plane = pitch   (planar: rowp = pitch,
//                                                         plane = (H+2*GHOST)*pitch);
// rho, u, v are [H][pitch]; the obstacle mask is uint8 [H + 2*LB_MASK_HALO_ROWS][pitch], row y at mask + y*pitch
// (7 rows of each neighbour).
// Source layout: d2q9_cell.h (cell arithmetic), kernels_fused.h (k_step, k_step2, k_step3), kernels_step4.h / 5 (k_step4,
// k_step5), kernels_deep.h (k_deep: six and seven steps per pass), kernels_tile.h (k_tile4, k_vel_band); every fused kernel family
// is instantiated in a translation unit of its own (launchers.h).  The host side is cut by concern (host.h): plan.cpp (what to launch:
// plain C++), launch.cpp (the launches), slab.cpp (halo exchange and the slab schedules), transport.cpp (RCCL, peer set-up),
// tune.cpp (lb_autotune*), and this file: the handle's life, state transfer, the un-fused phases and the Cython path
// (kernels_phases.h), the health check (kernels_check.h), lb_run's dispatch, lb_run_batch, timers.
// All stores of the fused kernel are 16-byte aligned; the six planes with cx != 0 are read through
// 16-byte loads that are misaligned by one element (gfx950 global loads only need dword alignment).
#include "host.h"

#include <cmath>
#include <initializer_list>
#include <stdarg.h>

#include "kernels_tile.h"       // TileLaunch, for k1_tile4
#include "kernels_phases.h"
#include "kernels_check.h"

static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

dim3 cells_grid(const lb_sim *s, int nz) { return dim3((s->p.nx + 255) / 256, s->p.ny, nz); }

PhaseArgs phase_args(const lb_sim *s)
{
    PhaseArgs a;
    a.f = s->origin(s->cur);
    a.fs = s->origin(s->cur ^ 1);
    a.feq = s->feq ? s->feq_origin() : nullptr;
    a.rho = s->rho; a.u = s->u; a.v = s->v;
    a.mask = s->has_mask ? s->mask : nullptr;
    a.plane = s->plane; a.pitch = (int)s->rowp; a.fpitch = (int)s->pitch; a.nx = s->p.nx; a.ny = s->p.ny; a.bc = kernel_bc(s);
    a.omega = s->p.omega; a.rho_in = s->p.inlet_rho; a.rho_out = s->p.outlet_rho;
    a.lid_u = s->p.lid_u; a.rho0 = s->p.rho0;
    a.u_w = s->p.inlet_u; a.u_e = s->p.outlet_u;
    return a;
}

int ensure_feq(lb_sim *s)
{
    if (s->feq) return LB_OK;
    HIP_TRY(hipMalloc(&s->feq, sizeof(float) * s->lat_floats));
    HIP_TRY(hipMemsetAsync(s->feq, 0, sizeof(float) * s->lat_floats, s->stream));
    s->bytes += sizeof(float) * s->lat_floats;
    return LB_OK;
}

int need_single_slab(const lb_sim *s, const char *what)
{
    if (s->multi_slab())
        return fail(LB_ERR_STATE, "%s is only available on a handle that owns the whole grid", what);
    return LB_OK;
}

// The health check's two passes on the handle's stream.  The first is the handle's kind's -- flow: k_macro_check over the current
// populations (store = rebuild rho, u, v from them on the way); scalar lattice: k_ad_check over the populations' sum and the imposed
// field -- and leaves one record per workgroup; k_check_final folds them into check_part[check_cap - 1], the record lb_check reads.
int check_pass(lb_sim *s, bool store)
{
    const StepArgs ad = step_args(s, 0, 1, s->H);       // (the scalar pass's arguments)
    const dim3 grid((unsigned)((s->pitch / 4 + 255) / 256), (unsigned)s->H);
    const long long blocks = s->scalar() ? ad_check_blocks(ad) : (long long)grid.x * grid.y;
    if (s->check_cap < blocks + 1) {
        if (s->check_part) HIP_TRY(hipFree(s->check_part));
        s->check_part = nullptr;
        s->check_cap = 0;
        HIP_TRY(hipMalloc(&s->check_part, sizeof(CheckPartial) * (size_t)(blocks + 1)));
        s->check_cap = blocks + 1;
        s->bytes += (int64_t)sizeof(CheckPartial) * (blocks + 1);
    }
    CheckPartial *part = s->check_part;
    if (s->scalar())
        lbk_ad_check(s->stream, ad, part);
    else if (store)
        hipLaunchKernelGGL(k_macro_check<true>, grid, dim3(256), 0, s->stream, (const float *)s->origin(s->cur), s->plane,
                           (int)s->rowp, (int)s->pitch, s->p.nx, s->rho, s->u, s->v, part);
    else
        hipLaunchKernelGGL(k_macro_check<false>, grid, dim3(256), 0, s->stream, (const float *)s->origin(s->cur), s->plane,
                           (int)s->rowp, (int)s->pitch, s->p.nx, s->rho, s->u, s->v, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_check_final, dim3(1), dim3(1024), 0, s->stream, (const CheckPartial *)part, blocks,
                       part + blocks);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// rho, u, v as of the last time step, before anybody reads them or overwrites the populations they are derived from
int ensure_macro(lb_sim *s)
{
    if (s->macro_valid) return LB_OK;
    // Only the families whose fields ARE the plain moments are ever rebuilt.  On the others (velocity inlet, D2Q9i, Cython
    // path) rho, u, v carry state the kernels read back (the inlet / outlet v, the corner u): a rebuild would overwrite it,
    // so a stale flag there -- e.g. left by a tuning pass that bailed out -- must never reach k_macro_check<STORE>.
    if (!lazy_macro(s)) {
        s->macro_valid = true;
        return LB_OK;
    }
    // (a run on a slab ends with both of its other streams joined into s->stream: lb_run's tail)
    int rc = check_pass(s, true);
    if (rc) return rc;
    s->macro_valid = true;
    return LB_OK;
}

// A whole lattice copied on the device by a kernel on the handle's stream (k_copy4: it runs at the streaming ceiling, and it
// is ordered like every other kernel of that stream; hipMemcpyAsync device-to-device goes through the runtime's copy path,
// whose completion the stream did not always wait for when several processes shared the GPU: tools/slab_stress.py).
int copy_lattice(lb_sim *s, float *dst, const float *src)
{
    const long long n4 = s->lat_floats / 4;              // (lat_floats is a multiple of 64)
    hipLaunchKernelGGL(k_copy4<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s->stream,
                       reinterpret_cast<const f4a *>(src), reinterpret_cast<f4a *>(dst), n4);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// host [rows][nx] <-> device [rows][pitch]
int copy_plane_h2d(lb_sim *s, float *dev, const float *host)
{
    HIP_TRY(hipMemcpy2DAsync(dev, s->pitch * sizeof(float), host, s->p.nx * sizeof(float),
                             s->p.nx * sizeof(float), s->H, hipMemcpyHostToDevice, s->stream));
    return LB_OK;
}
int copy_plane_d2h(lb_sim *s, float *host, const float *dev)
{
    HIP_TRY(hipMemcpy2DAsync(host, s->p.nx * sizeof(float), dev, s->pitch * sizeof(float),
                             s->p.nx * sizeof(float), s->H, hipMemcpyDeviceToHost, s->stream));
    return LB_OK;
}

// One plane of a lattice (f or feq; `origin` = its plane 0, row 0): host [H][nx] <-> device.  Planar layout: the plane is one
// pitched block.  Interleaved rows: through the staging plane -- one DMA plus one device kernel instead of H strided
// row copies.  The staging plane is reused plane after plane; the stream is synchronised between the scatter / gather
// kernel and the next copy from / to (pageable) host memory instead of relying on the runtime ordering its staged copies
// behind kernels already enqueued -- a precaution (nine cheap synchronisations per set / get), not a measured necessity.
int lattice_plane_h2d(lb_sim *s, float *origin, int k, const float *host)
{
    if (s->rowp == s->pitch) return copy_plane_h2d(s, origin + k * s->plane, host);
    if (!s->stage) HIP_TRY(hipMalloc(&s->stage, sizeof(float) * s->pitch * s->H));
    int rc = copy_plane_h2d(s, s->stage, host);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));           // the upload has landed
    const dim3 grid((unsigned)((s->pitch / 4 + 255) / 256), (unsigned)s->H, 1);
    hipLaunchKernelGGL(k_rows_copy, grid, dim3(256), 0, s->stream, (const float *)s->stage, origin + k * s->plane, 0LL, 0LL,
                       (int)s->pitch, s->pitch, s->rowp, s->H, 0, 0, 0, 0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));           // the staging plane is free again
    return LB_OK;
}
int lattice_plane_d2h(lb_sim *s, float *host, const float *origin, int k)
{
    if (s->rowp == s->pitch) return copy_plane_d2h(s, host, origin + k * s->plane);
    if (!s->stage) HIP_TRY(hipMalloc(&s->stage, sizeof(float) * s->pitch * s->H));
    const dim3 grid((unsigned)((s->pitch / 4 + 255) / 256), (unsigned)s->H, 1);
    hipLaunchKernelGGL(k_rows_copy, grid, dim3(256), 0, s->stream, origin + k * s->plane, s->stage, 0LL, 0LL, (int)s->pitch,
                       s->rowp, s->pitch, s->H, 0, 0, 0, 0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));           // the staging plane is complete
    int rc = copy_plane_d2h(s, host, s->stage);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));           // ... and read, before the next plane is gathered into it
    return LB_OK;
}

// Links no kernel ever writes keep the value they had when the populations were last set as a whole (the reference's f_streamed = f
// at that moment: opencl_dim.py:323-327, diffusion.py:321-324): the eight corner links of the VELOCITY_INLET family and the eight of
// a coupled scalar lattice's LB_BC_BOX (vi_corner), the edge state of a scalar lattice's OPEN family (ad_edge, scalar_launch.h); no other handle has any.  They are kept apart because
// fused launches swap the lattices, so "whatever f_streamed held" would not survive them.  !patch: copied out of lattice `which`;
// patch: written back into it.
int frozen_links(lb_sim *s, int which, bool patch)
{
    if (s->p.bc_mode == LB_BC_VELOCITY_INLET || s->p.bc_mode == LB_BC_BOX || s->p.bc_mode == LB_BC_DIRICHLET) {
        const int X = s->p.nx - 1, Y = s->p.ny - 1;
        struct Link { int k, x, y; };
        const Link vel[8] = {{1, 0, 0}, {8, 0, 0}, {1, 0, Y}, {5, 0, Y}, {3, X, 0}, {7, X, 0}, {3, X, Y}, {6, X, Y}};   // (bc_vel_cell's order)
        const Link box[8] = {{6, 0, 0}, {8, 0, 0}, {5, X, 0}, {7, X, 0}, {5, 0, Y}, {7, 0, Y}, {6, X, Y}, {8, X, Y}};   // (mf_box_cell's and ps_box_cell's order)
        const Link *c = s->p.bc_mode == LB_BC_VELOCITY_INLET ? vel : box;
        for (int i = 0; i < 8; ++i) {
            float *in_lat = s->origin(which) + c[i].k * s->plane + (long long)c[i].y * s->rowp + c[i].x, *kept = s->vi_corner + i;
            HIP_TRY(hipMemcpyAsync(patch ? in_lat : kept, patch ? kept : in_lat, sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        }
    } else if (s->ad_edge) {
        const StepArgs a = step_args(s, 0, 1, s->H);
        if (patch) lbk_ad_edge_patch(s->stream, a, s->origin(which), s->ad_edge);
        else lbk_ad_edge_capture(s->stream, a, s->origin(which), s->ad_edge);
        HIP_TRY(hipGetLastError());
    }
    return LB_OK;
}
// ... whenever the populations are set as a whole (lb_set_f, lb_init_pop)
int frozen_capture(lb_sim *s, int which) { return frozen_links(s, which, false); }
// ... behind the un-fused streaming phase (lb_move), where the boundary phase reads them
int frozen_patch(lb_sim *s, int which) { return frozen_links(s, which, true); }

// ABI order of the edge state (include/lb_hip.h: west, east, south, north; unpadded) <-> device order (scalar_launch.h)
long long edge_host_floats(const lb_sim *s) { return s->ad_edge ? 6LL * (s->p.nx + s->p.ny) : 0; }

// lb_run in Cython-path semantics
int run_cython(lb_sim *s, int n_steps)
{
    // cython_dim.pyx:346-359: move_bcs, move, update_hydro, update_feq, collide_particles.  The boundary phase of the
    // FIRST step in place (k1_bcs); then one pass per step (k1_fstep: restricted pull, moments with their overrides,
    // equilibrium, relaxation and -- all but the last -- the NEXT step's boundary rule on the cells it concerns, which
    // only needs what the pass has in registers); bitwise equal to the five phase calls per step
    // (test_cython_path_fused_run_equals_phase_calls)
    if (n_steps > 0) {
        hipLaunchKernelGGL(k1_bcs, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
        HIP_TRY(hipGetLastError());
    }
    // n = 4a + rem: the remainder first, step by step (k1_fstep: four cells per lane, 16-byte accesses, at the streaming
    // ceiling of a pass that moves 72 B per cell), then a launches of four steps each through LDS tiles (k1_tile4);
    // grids too small for tiles, or LB_VARIANT / lb_set_variant without LB_VAR_TILES with an explicit variant: single steps only
    const dim3 blk(64, 4), grd((unsigned)((s->pitch / 4 + 63) / 64), (unsigned)((s->H + 3) / 4));
    // (rounds 4-5 also had a five-step marching form, k1_step5: bitwise right, slower than the tiles at the reference's sizes --
    //  3751 x 1251 with the cylinder 136 against 174 k MLUPS --, diagnostic build only in round 5, removed in round 6)
    const bool tiles = cython_tiles(s);
    int left = n_steps;
    while (left > 0) {
        const PhaseArgs a = phase_args(s);
        if (tiles && left % TILE_T == 0) {
            const TileLaunch<32, 16, 2> t(s->p.nx, s->H);
            const bool lastp = (left == TILE_T);
#define LB_LAUNCH1T(MASK)                                                                                                  \
            do {                                                                                                       \
                if (lastp) hipLaunchKernelGGL((k1_tile4<MASK, true, false>), t.grid, t.block, 0, s->stream, a, t.tiles_x, t.n_tiles); \
                else hipLaunchKernelGGL((k1_tile4<MASK, false, true>), t.grid, t.block, 0, s->stream, a, t.tiles_x, t.n_tiles);       \
            } while (0)
            if (s->has_mask) LB_LAUNCH1T(true); else LB_LAUNCH1T(false);
#undef LB_LAUNCH1T
            left -= TILE_T;
        } else {
            const bool lastp = (left == 1);
            if (s->has_mask) {
                if (lastp) hipLaunchKernelGGL((k1_fstep<true, false, true>), grd, blk, 0, s->stream, a);
                else hipLaunchKernelGGL((k1_fstep<true, true, false>), grd, blk, 0, s->stream, a);
            } else {
                if (lastp) hipLaunchKernelGGL((k1_fstep<false, false, true>), grd, blk, 0, s->stream, a);
                else hipLaunchKernelGGL((k1_fstep<false, true, false>), grd, blk, 0, s->stream, a);
            }
            left -= 1;
        }
        HIP_TRY(hipGetLastError());
        s->cur ^= 1;
    }
    if (n_steps) { s->feq_valid = false; s->macro_valid = true; }
    return LB_OK;
}

}  // namespace

extern "C" {

int lb_abi_version(void) { return LB_ABI_VERSION; }

const char *lb_last_error(void) { return g_err; }

int lb_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(LB_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int lb_create(const lb_params *p, lb_sim **out)
{
    if (!p || !out) return fail(LB_ERR_ARG, "null argument");
    *out = nullptr;
    if (p->nx < 2 || p->ny < 2) return fail(LB_ERR_ARG, "grid must be at least 2x2 (got %dx%d)", p->nx, p->ny);
    if (p->local_ny < 1 || p->y0 < 0 || p->y0 + p->local_ny > p->ny)
        return fail(LB_ERR_ARG, "slab [%d,%d) outside 0..%d", p->y0, p->y0 + p->local_ny, p->ny);
    if (p->bc_mode < LB_BC_PIPE || p->bc_mode > LB_BC_ZERO_GRADIENT) return fail(LB_ERR_ARG, "unknown bc_mode %d", p->bc_mode);
    if (p->bc_mode == LB_BC_ZERO_GRADIENT && p->semantics != LB_SEM_POROUS && p->semantics != LB_SEM_MULTIFLUID)
        return fail(LB_ERR_ARG, "LB_BC_ZERO_GRADIENT exists for forced flow in a porous medium (LB_SEM_POROUS) only: unknown bc_mode %d for semantics %d", p->bc_mode, p->semantics);
    if (p->bc_mode == LB_BC_DIRICHLET && p->semantics != LB_SEM_POISSON)
        return fail(LB_ERR_ARG, "LB_BC_DIRICHLET exists for the LB Poisson solver (LB_SEM_POISSON) only: unknown bc_mode %d for semantics %d", p->bc_mode, p->semantics);
    if (p->semantics == LB_SEM_POISSON) {
        // the LB Poisson solver: a scalar lattice, refused likewise (before any device is touched)
        if (p->bc_mode != LB_BC_DIRICHLET)
            return fail(LB_ERR_ARG, "the LB Poisson solver (LB_SEM_POISSON) takes the family LB_BC_DIRICHLET only: unknown semantics %d for bc_mode %d", p->semantics, p->bc_mode);
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "the LB Poisson solver (LB_SEM_POISSON) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "the LB Poisson solver (LB_SEM_POISSON) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "the LB Poisson solver (LB_SEM_POISSON) runs on a GPU only (no CPU backend)");
    }
    if (p->semantics == LB_SEM_POROUS) {
        // the porous-medium fluid: a whole-grid GPU handle without obstacles, refused like the scalar lattices (before any device is touched)
        if (p->bc_mode != LB_BC_PERIODIC && p->bc_mode != LB_BC_ZERO_GRADIENT)
            return fail(LB_ERR_ARG, "forced flow in a porous medium (LB_SEM_POROUS) takes the families LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT only");
        if (p->bc_mode == LB_BC_ZERO_GRADIENT && (p->nx < 3 || p->ny < 3))
            return fail(LB_ERR_ARG, "LB_BC_ZERO_GRADIENT needs an interior cell: grid must be at least 3x3 (got %dx%d)", p->nx, p->ny);
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "forced flow in a porous medium (LB_SEM_POROUS) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "forced flow in a porous medium (LB_SEM_POROUS) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "forced flow in a porous medium (LB_SEM_POROUS) runs on a GPU only (no CPU backend)");
    }
    if (p->semantics == LB_SEM_MULTIFLUID) {
        // a fluid of a multicomponent set: a whole-grid GPU handle without obstacles, refused likewise
        if (p->bc_mode != LB_BC_PERIODIC && p->bc_mode != LB_BC_ZERO_GRADIENT)
            return fail(LB_ERR_ARG, "a fluid of a multicomponent set (LB_SEM_MULTIFLUID) takes the families LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT only");
        if (p->nx < 3 || p->ny < 3)
            return fail(LB_ERR_ARG, "a fluid of a multicomponent set (LB_SEM_MULTIFLUID) needs a cell with eight neighbours: grid must be at least 3x3 (got %dx%d)", p->nx, p->ny);
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "a fluid of a multicomponent set (LB_SEM_MULTIFLUID) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "a fluid of a multicomponent set (LB_SEM_MULTIFLUID) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "a fluid of a multicomponent set (LB_SEM_MULTIFLUID) runs on a GPU only (no CPU backend)");
    }
    if (p->semantics == LB_SEM_ROCKET) {
        // a lattice of a surfactant-propelled colony: a whole-grid GPU scalar lattice, refused likewise
        if (p->bc_mode != LB_BC_PERIODIC)
            return fail(LB_ERR_ARG, "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) takes the family LB_BC_PERIODIC only (box boundaries are not built)");
        if (p->nx < 3 || p->ny < 3)
            return fail(LB_ERR_ARG, "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) needs a cell with eight neighbours: grid must be at least 3x3 (got %dx%d)", p->nx, p->ny);
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) runs on a GPU only (no CPU backend)");
    }
    if (p->bc_mode == LB_BC_OPEN && p->semantics != LB_SEM_DIFFUSION)
        return fail(LB_ERR_ARG, "LB_BC_OPEN exists for scalar lattices (LB_SEM_DIFFUSION) only");
    if (p->bc_mode == LB_BC_BOX && p->semantics != LB_SEM_MULTIFIELD)
        return fail(LB_ERR_ARG, "bc_mode LB_BC_BOX exists for coupled scalar lattices (LB_SEM_MULTIFIELD) only");
    if (p->semantics == LB_SEM_MULTIFIELD) {
        // the fields of a coupled set: scalar lattices, refused likewise
        if (p->bc_mode != LB_BC_PERIODIC && p->bc_mode != LB_BC_BOX)
            return fail(LB_ERR_ARG, "a coupled scalar lattice (LB_SEM_MULTIFIELD) takes the families LB_BC_PERIODIC and LB_BC_BOX only");
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "a coupled scalar lattice (LB_SEM_MULTIFIELD) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "a coupled scalar lattice (LB_SEM_MULTIFIELD) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "a coupled scalar lattice (LB_SEM_MULTIFIELD) runs on a GPU only (no CPU backend)");
    }
    if (p->semantics == LB_SEM_DIFFUSION) {
        // scalar lattices (refused before any device is touched)
        if (p->bc_mode != LB_BC_PERIODIC && p->bc_mode != LB_BC_OPEN)
            return fail(LB_ERR_ARG, "a scalar lattice (LB_SEM_DIFFUSION) takes the families LB_BC_PERIODIC and LB_BC_OPEN only");
        if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "a scalar lattice (LB_SEM_DIFFUSION) owns its whole grid: no slabs");
        if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "a scalar lattice (LB_SEM_DIFFUSION) has no halo interface (LB_FLAG_HALO)");
        if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "a scalar lattice (LB_SEM_DIFFUSION) runs on a GPU only (no CPU backend)");
    }
    if (p->bc_mode == LB_BC_VELOCITY_INLET &&
        (p->local_ny != p->ny || (p->flags & LB_FLAG_HALO) || p->semantics != LB_SEM_OPENCL))
        return fail(LB_ERR_ARG, "the velocity-inlet family exists for whole-grid OpenCL-path handles only");
    if (p->bc_mode == LB_BC_VELOCITY_INLET && (!(p->inlet_u < 1.f) || !(p->outlet_u > -1.f)))
        return fail(LB_ERR_ARG, "velocity-inlet speeds must satisfy inlet_u < 1 and outlet_u > -1");
    if (!(p->omega > 0.f && p->omega < 2.f)) return fail(LB_ERR_ARG, "omega must be in (0,2), got %g", p->omega);
    for (int r : p->reserved)
        if (r != 0) return fail(LB_ERR_ARG, "reserved fields must be zero");
    if (p->flags & ~(LB_FLAG_HALO | LB_FLAG_PLANAR | LB_FLAG_EAGER_MACRO)) return fail(LB_ERR_ARG, "unknown flags 0x%x", p->flags);
    if (p->semantics != LB_SEM_OPENCL && p->semantics != LB_SEM_CYTHON && p->semantics != LB_SEM_OPENCL_D2Q9I && p->semantics != LB_SEM_DIFFUSION &&
        p->semantics != LB_SEM_MULTIFIELD && p->semantics != LB_SEM_POISSON && p->semantics != LB_SEM_POROUS && p->semantics != LB_SEM_MULTIFLUID &&
        p->semantics != LB_SEM_ROCKET)
        return fail(LB_ERR_ARG, "unknown semantics %d", p->semantics);
    if (p->semantics == LB_SEM_OPENCL_D2Q9I &&
        (p->bc_mode != LB_BC_PIPE || p->local_ny != p->ny || (p->flags & LB_FLAG_HALO)))
        return fail(LB_ERR_ARG, "the D2Q9i fork exists for whole-grid pipe-flow handles only");
    if (p->semantics == LB_SEM_CYTHON &&
        (p->bc_mode != LB_BC_PIPE || p->local_ny != p->ny || (p->flags & LB_FLAG_HALO)))
        return fail(LB_ERR_ARG, "Cython-path semantics exist for whole-grid pipe-flow handles only");
    if (p->device == LB_DEVICE_CPU) {
        // the CPU backend: asked for by name, never chosen for the caller (include/lb_hip.h, LB_DEVICE_CPU)
        if (p->semantics != LB_SEM_CYTHON || p->bc_mode != LB_BC_PIPE || p->local_ny != p->ny || p->y0 != 0 || p->flags != 0)
            return fail(LB_ERR_ARG, "the CPU backend runs whole-grid pipe flow in Cython-path semantics (LB_SEM_CYTHON) only");
        lb_sim *s = new lb_sim();
        s->p = *p;
        s->H = p->ny;
        s->cpu = new lbcpu::CpuPipe();
        s->cpu->resize(p->nx, p->ny);
        s->cpu->omega = (double)p->omega;           // (the ABI carries float32 parameters: the reference's np.float64 values
        s->cpu->rho_in = (double)p->inlet_rho;      //  rounded once, as on the GPU path)
        s->cpu->rho_out = (double)p->outlet_rho;
        *out = s;
        return LB_OK;
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(LB_ERR_HIP, "no HIP device visible");
    if (p->device < 0 || p->device >= ndev) return fail(LB_ERR_ARG, "device %d not in 0..%d", p->device, ndev - 1);

    DeviceGuard guard(p->device);
    lb_sim *s = new lb_sim();
    s->p = *p;
    s->H = p->local_ny;
    s->pitch = ((long long)p->nx + 63) / 64 * 64;
    // (padding the row pitch or skewing the plane stride away from powers of two was measured:
    //  no gain for k_step2, -5..-8 % for k_step -- profiles/r01_sweep_variants.txt)
    if (p->flags & LB_FLAG_PLANAR) {
        s->rowp = s->pitch;
        s->plane = (long long)(s->H + 2 * GHOST) * s->pitch;
    } else {
        s->rowp = 9 * s->pitch;
        s->plane = s->pitch;
    }
    s->lat_floats = 9 * (long long)(s->H + 2 * GHOST) * s->pitch + 2 * GUARD;
    if (const char *e = getenv("LB_VARIANT")) s->variant = atoi(e);
    if (const char *e = getenv("LB_DIAG")) s->diag = atoi(e);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0)
            s->cu_count = prop.multiProcessorCount;
    }

#define CREATE_TRY(expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fail(LB_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                   \
            lb_destroy(s);                                                                     \
            return LB_ERR_HIP;                                                                 \
        }                                                                                      \
    } while (0)
    CREATE_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    // (Three streams that must not share a hardware queue -- interior, edge bands, halo exchange.  HIP maps a process's streams onto
    //  GPU_MAX_HW_QUEUES queues, four by default, per priority, and not once and for all: a probe at creation saw three queues in a
    //  process whose timeline later shows the exchange on the interior's queue.  The process decides -- bench.py sets 8 --; a
    //  communication stream at the highest priority, a queue pool of its own, pushed the EDGE stream onto the interior's queue in
    //  bench.py's process structure, 370 -> 230 k MLUPS: profiles/r06_experiments.txt section 10c, r06h_bench_comm_prio.txt.)
    CREATE_TRY(hipStreamCreateWithFlags(&s->comm_stream, hipStreamNonBlocking));
    // The edge stream (edge bands, halo push / RCCL) at NORMAL priority, like the other two.  Rounds 1-2 created it at the
    // device's highest priority; with it, ~2 % of random slab partitions run through lb_run_group with events alone differed from
    // the undivided run when four other processes kept the GPU busy (17 of ~900, tools/slab_stress.py), none of 1650 without,
    // while a stand-alone stress of HIP's cross-queue ordering finds nothing (tools/queue_order_repro.hip) and an audit of
    // every read-after-write and write-after-read pair of the cycle finds every one ordered.  The
    // priority bought nothing measurable (profiles/r03_experiments.txt section 6), so there is no such stream and no switch for one.
    // (Rounds 3-5 passed the FIRST value hipDeviceGetStreamPriorityRange returns -- the LEAST priority, not the normal one the
    //  comment claimed: the edge bands, which gate the halo, ran on a low-priority queue.  Round 6: no priority argument at all.)
    CREATE_TRY(hipStreamCreateWithFlags(&s->edge_stream, hipStreamNonBlocking));
    const unsigned ev_flags = hipEventDisableTiming;
    CREATE_TRY(hipEventCreateWithFlags(&s->ev_boundary, ev_flags));
    CREATE_TRY(hipEventCreateWithFlags(&s->ev_halo, ev_flags));
    CREATE_TRY(hipEventCreateWithFlags(&s->ev_interior, ev_flags));
    CREATE_TRY(hipEventCreateWithFlags(&s->ev_packed, ev_flags));
    CREATE_TRY(hipEventCreateWithFlags(&s->ev_edge, ev_flags));
    CREATE_TRY(hipEventCreate(&s->ev_t0));
    CREATE_TRY(hipEventCreate(&s->ev_t1));
    const size_t lat_bytes = sizeof(float) * s->lat_floats;
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    for (int i = 0; i < 2; ++i) {
        CREATE_TRY(hipMalloc(&s->lat[i], lat_bytes));
        CREATE_TRY(hipMemsetAsync(s->lat[i], 0, lat_bytes, s->stream));
    }
    CREATE_TRY(hipMalloc(&s->rho, fld_bytes));
    CREATE_TRY(hipMalloc(&s->u, fld_bytes));
    CREATE_TRY(hipMalloc(&s->v, fld_bytes));
    if (s->scalar() && p->bc_mode == LB_BC_OPEN) {
        const size_t edge_bytes = sizeof(float) * (size_t)ad_edge_device_floats(s->pitch, p->ny);
        CREATE_TRY(hipMalloc(&s->ad_edge, edge_bytes));
        CREATE_TRY(hipMemsetAsync(s->ad_edge, 0, edge_bytes, s->stream));
    }
    if (s->poisson()) {
        // (the diagnostic word of the flow kernels means nothing here: on this handle it is lb_solve's batch length)
        s->ps_batch = s->diag > 0 ? s->diag : 0;
        s->diag = 0;
        const size_t part_bytes = 2 * sizeof(float) * (size_t)ps_step_blocks(step_args(s, 0, 1, s->H));
        CREATE_TRY(hipMalloc(&s->ps_source, fld_bytes));
        CREATE_TRY(hipMemsetAsync(s->ps_source, 0, fld_bytes, s->stream));
        CREATE_TRY(hipMalloc(&s->ps_part, part_bytes));
        CREATE_TRY(hipMemsetAsync(s->ps_part, 0, part_bytes, s->stream));
        CREATE_TRY(hipMalloc(&s->ps_state, sizeof(PsState)));
        const PsState fresh = {0, nanf(""), 0, 0};
        CREATE_TRY(hipMemcpy(s->ps_state, &fresh, sizeof(fresh), hipMemcpyHostToDevice));
        s->bytes += fld_bytes + part_bytes + sizeof(PsState);
    }
    if (s->porous() || s->multifluid() || s->rocket()) {
        s->diag = 0;                                // (the diagnostic word of the flow kernels means nothing here)
        for (float **q : {&s->pm_G[0], &s->pm_G[1], &s->pm_ub[0], &s->pm_ub[1]}) {
            CREATE_TRY(hipMalloc(q, fld_bytes));
            CREATE_TRY(hipMemsetAsync(*q, 0, fld_bytes, s->stream));
        }
        s->bytes += 4 * fld_bytes;
    }
    if (s->rocket()) {
        // (every handle can be a set's first: psi / S and the forces of the last step live there)
        CREATE_TRY(hipMalloc(&s->ry_op, fld_bytes));
        CREATE_TRY(hipMemsetAsync(s->ry_op, 0, fld_bytes, s->stream));
        s->bytes += fld_bytes;
    }
    CREATE_TRY(hipMalloc(&s->vi_corner, 8 * sizeof(float)));
    CREATE_TRY(hipMemsetAsync(s->vi_corner, 0, 8 * sizeof(float), s->stream));
    CREATE_TRY(hipMalloc(&s->mask_raw, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD));
    s->mask = s->mask_raw + GUARD + MASK_GHOST * s->pitch;
    CREATE_TRY(hipMemsetAsync(s->rho, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->u, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->v, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->mask_raw, 0, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD, s->stream));
    CREATE_TRY(hipStreamSynchronize(s->stream));
#undef CREATE_TRY
    s->bytes += 2 * lat_bytes + 3 * fld_bytes + (size_t)s->pitch * s->H;
    // A periodic box whose width is not a multiple of 4 cannot use the marching kernels (their lanes hold four consecutive
    // cells, and the wrap at x = nx must fall on a lane boundary): above the Infinity Cache that costs a factor of two or
    // more (LDS tiles / single steps instead of k_step5 / k_step6).  Say so once instead of being silently slow; LB_QUIET=1 mutes it.
    if (p->bc_mode == LB_BC_PERIODIC && (p->nx % 4) != 0 && (double)p->nx * s->H >= 1950.0 * 1950.0) {
        static bool warned = false;
        if (!warned && !(getenv("LB_QUIET") && atoi(getenv("LB_QUIET")) != 0)) {
            warned = true;
            fprintf(stderr, "liblbhip: periodic grid %d x %d: nx is not a multiple of 4, so the multi-step marching kernels do "
                            "not apply and this grid runs on the slower tile / single-step kernels (pad nx to a multiple of 4 "
                            "for full speed).\n", p->nx, p->ny);
        }
    }
    *out = s;
    return LB_OK;
}

int lb_destroy(lb_sim *s)
{
    if (s && s->cpu) {
        delete s->cpu;
        delete s;
        return LB_OK;
    }
    if (!s) return LB_OK;
    DeviceGuard guard(s->p.device);
    if (s->own_stream) (void)hipStreamSynchronize(s->own_stream);
    if (s->comm_stream) (void)hipStreamSynchronize(s->comm_stream);
    if (s->edge_stream) (void)hipStreamSynchronize(s->edge_stream);
    drop_graph(s);
    for (hipEvent_t e : s->xt_ev)
        if (e) (void)hipEventDestroy(e);
    for (lb_sim::PeerNb &nb : s->peer_nb)
        if (nb.mapped) {
            (void)hipIpcCloseMemHandle(nb.flags);
            for (float *l : nb.lat_raw)
                if (l) (void)hipIpcCloseMemHandle(l);
        }
    if (s->peer_flags) (void)hipFree(s->peer_flags);
    if (s->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(s->comm);
    for (float *p : {s->lat[0], s->lat[1], s->feq, s->rho, s->u, s->v, s->halo_buf, s->vi_corner, s->stage, s->ad_edge, s->ps_source, s->ps_part,
                     s->pm_G[0], s->pm_G[1], s->pm_ub[0], s->pm_ub[1], s->pm_field[0], s->pm_field[1], s->ry_op})
        if (p) (void)hipFree(p);
    if (s->mask_raw) (void)hipFree(s->mask_raw);
    if (s->check_part) (void)hipFree(s->check_part);
    if (s->ps_state) (void)hipFree(s->ps_state);
    for (hipEvent_t e : {s->ev_boundary, s->ev_interior, s->ev_halo, s->ev_packed, s->ev_edge, s->ev_t0, s->ev_t1})
        if (e) (void)hipEventDestroy(e);
    if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
    if (s->comm_stream) (void)hipStreamDestroy(s->comm_stream);
    if (s->edge_stream) (void)hipStreamDestroy(s->edge_stream);
    delete s;
    return LB_OK;
}

int lb_set_params_f64(lb_sim *s, double omega, double inlet_rho, double outlet_rho)
{
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (!s->cpu) return fail(LB_ERR_STATE, "lb_set_params_f64 is for handles of the CPU backend (the device kernels compute in float32)");
    if (!(omega > 0. && omega < 2.)) return fail(LB_ERR_ARG, "omega must be in (0,2), got %g", omega);
    s->cpu->omega = omega;
    s->cpu->rho_in = inlet_rho;
    s->cpu->rho_out = outlet_rho;
    return LB_OK;
}

int lb_sync(lb_sim *s)
{
    if (s && s->cpu) return LB_OK;                 // (the host backend is synchronous)
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->comm_stream));
    HIP_TRY(hipStreamSynchronize(s->edge_stream));
    return peer_check_error(s);
}

int lb_set_stream(lb_sim *s, void *hip_stream)
{
    CPU_UNSUPPORTED(s, "lb_set_stream");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->stream = hip_stream ? (hipStream_t)hip_stream : s->own_stream;
    return LB_OK;
}

int lb_set_variant(lb_sim *s, int variant)
{
    if (s && s->cpu) return LB_OK;                 // (one code path: nothing to select)
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->multifield() && variant != -1 && variant != 0)
        return fail(LB_ERR_ARG, "a coupled scalar lattice (LB_SEM_MULTIFIELD) takes the variants -1 and 0 only: k_mf_step, no tiles");
    if (s->poisson() && variant != -1 && variant != 0)
        return fail(LB_ERR_STATE, "the LB Poisson solver (LB_SEM_POISSON) takes the variants -1 and 0 only: k_ps_step, no tiles");
    if (s->porous() && variant != -1 && variant != 0)
        return fail(LB_ERR_STATE, "lb_set_variant: a porous-medium fluid (LB_SEM_POROUS) takes the variants -1 and 0 only: k_pm_step, no tiles");
    if (s->multifluid() && (variant < -1 || variant > 1))
        return fail(LB_ERR_STATE, "lb_set_variant: a fluid of a multicomponent set (LB_SEM_MULTIFLUID) takes the variants -1 (the planner's choice), 0 (the two-launch step k_mc_moments + k_mc_collide) and 1 (the one-launch step k_mc_step) only");
    if (s->rocket() && (variant < -1 || variant > 1))
        return fail(LB_ERR_STATE, "lb_set_variant: a lattice of a surfactant-propelled colony (LB_SEM_ROCKET) takes the variants -1 (the planner's choice), 0 (the two-launch step k_ry_moments + k_ry_collide) and 1 (the one-launch step k_ry_step) only");
    s->variant = variant;
    return LB_OK;
}

int lb_set_slab_cycle(lb_sim *s, int depth)
{
    if (s && s->cpu) return LB_OK;
    SCALAR_UNSUPPORTED(s, "lb_set_slab_cycle");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    // (8: the seven-step cycle with k_deep2<7> for its launches, 7: with k_deep<7>; 0: automatic depth, kernel by transport)
    if (depth != 0 && (depth < 3 || depth > MAX_DEPTH + 1))
        return fail(LB_ERR_ARG, "halo cycle depth must be 0 (automatic), 3..%d, or %d (seven steps by k_deep2), got %d", MAX_DEPTH, MAX_DEPTH + 1, depth);
    s->forced_cycle = depth > MAX_DEPTH ? MAX_DEPTH : depth;
    s->slab_flavour = depth == 0 ? -1 : (depth > MAX_DEPTH ? 1 : 0);
    return LB_OK;
}

int lb_set_exchange_inline(lb_sim *s, int on)
{
    if (s && s->cpu) return LB_OK;
    SCALAR_UNSUPPORTED(s, "lb_set_exchange_inline");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    s->xchg_inline = on != 0;
    return LB_OK;
}

int lb_exchange_timing(lb_sim *s, int enable)
{
    CPU_UNSUPPORTED(s, "lb_exchange_timing");
    SCALAR_UNSUPPORTED(s, "lb_exchange_timing");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    if (enable && !s->xt_ev[0])
        for (hipEvent_t &e : s->xt_ev) HIP_TRY(hipEventCreate(&e));
    s->xt_on = enable != 0;
    s->xt_count = s->xt_dropped = 0;
    return LB_OK;
}

int lb_exchange_stats(lb_sim *s, int64_t *n_exchanges, double *total_ms, double *max_ms, int *cycle_depth_out, int *band_rows)
{
    CPU_UNSUPPORTED(s, "lb_exchange_stats");
    SCALAR_UNSUPPORTED(s, "lb_exchange_stats");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    double total = 0., mx = 0.;
    for (int i = 0; i < s->xt_count; ++i) {
        HIP_TRY(hipEventSynchronize(s->xt_ev[2 * i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->xt_ev[2 * i], s->xt_ev[2 * i + 1]));
        total += ms;
        mx = std::max(mx, (double)ms);
    }
    if (n_exchanges) *n_exchanges = s->xt_count;
    if (total_ms) *total_ms = total;
    if (max_ms) *max_ms = mx;
    const int D = s->multi_slab() ? cycle_depth(s, s->agreed_h()) : 0;
    if (cycle_depth_out) *cycle_depth_out = D;
    if (band_rows) *band_rows = D ? 2 * D + band_extra(s, D, true) : 0;
    s->xt_count = s->xt_dropped = 0;
    return LB_OK;
}

int lb_layout(lb_sim *s, int64_t *pitch, int64_t *plane_stride, int64_t *bytes_allocated)
{
    if (s && s->cpu) {
        if (pitch) *pitch = s->cpu->nx;
        if (plane_stride) *plane_stride = (int64_t)s->cpu->plane();
        if (bytes_allocated) *bytes_allocated = (int64_t)s->cpu->plane() * (18 * 4 + 4 + 16 + 1);
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (pitch) *pitch = s->pitch;
    if (plane_stride) *plane_stride = s->plane;
    if (bytes_allocated) *bytes_allocated = s->bytes;
    return LB_OK;
}

// ---- state transfer ----------------------------------------------------------------------
int lb_set_macro(lb_sim *s, const float *rho, const float *u, const float *v)
{
    if (s && s->cpu) {
        if (!rho || !u || !v) return fail(LB_ERR_ARG, "null argument");
        const size_t n = s->cpu->plane();
        for (size_t c = 0; c < n; ++c) { s->cpu->rho[c] = rho[c]; s->cpu->u[c] = u[c]; s->cpu->v[c] = v[c]; }
        return LB_OK;
    }
    if (!s || !rho || !u || !v) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc;
    s->macro_valid = true;
    if ((rc = copy_plane_h2d(s, s->rho, rho))) return rc;
    if ((rc = copy_plane_h2d(s, s->u, u))) return rc;
    if ((rc = copy_plane_h2d(s, s->v, v))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_get_macro(lb_sim *s, float *rho, float *u, float *v)
{
    if (s && s->cpu) {
        const size_t n = s->cpu->plane();
        for (size_t c = 0; c < n; ++c) {
            if (rho) rho[c] = s->cpu->rho[c];
            if (u) u[c] = (float)s->cpu->u[c];
            if (v) v[c] = (float)s->cpu->v[c];
        }
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    int rc;
    if ((rc = ensure_macro(s))) return rc;
    if (rho && (rc = copy_plane_d2h(s, rho, s->rho))) return rc;
    if (u && (rc = copy_plane_d2h(s, u, s->u))) return rc;
    if (v && (rc = copy_plane_d2h(s, v, s->v))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_set_f(lb_sim *s, const float *f)
{
    if (s && s->cpu) {
        if (!f) return fail(LB_ERR_ARG, "null argument");
        memcpy(s->cpu->f.data(), f, sizeof(float) * 9 * s->cpu->plane());
        return LB_OK;
    }
    if (!s || !f) return fail(LB_ERR_ARG, "null argument");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_set_f between lb_step_boundary and lb_step_finish");
    DeviceGuard guard(s->p.device);
    int rc = ensure_macro(s);       // rho, u, v stay those of the last step, as in the reference (they are derived from the OLD f)
    if (rc) return rc;
    const size_t host_plane = (size_t)s->p.nx * s->H;
    for (int k = 0; k < 9; ++k) {
        rc = lattice_plane_h2d(s, s->origin(s->cur), k, f + k * host_plane);
        if (rc) return rc;
    }
    // f_streamed = f (opencl_dim.py:323-327)
    rc = copy_lattice(s, s->lat[s->cur ^ 1], s->lat[s->cur]);
    if (rc) return rc;
    if ((rc = frozen_capture(s, s->cur))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->ghost_depth = 0;
    return LB_OK;
}

int lb_get_f(lb_sim *s, float *f)
{
    if (s && s->cpu) {
        if (!f) return fail(LB_ERR_ARG, "null argument");
        memcpy(f, s->cpu->f.data(), sizeof(float) * 9 * s->cpu->plane());
        return LB_OK;
    }
    if (!s || !f) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->comm_stream));
    const size_t host_plane = (size_t)s->p.nx * s->H;
    for (int k = 0; k < 9; ++k) {
        int rc = lattice_plane_d2h(s, f + k * host_plane, s->origin(s->cur), k);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_get_corner_state(lb_sim *s, float *out8)
{
    CPU_UNSUPPORTED(s, "lb_get_corner_state");
    if (s && !s->multifield() && !s->poisson()) SCALAR_UNSUPPORTED(s, "lb_get_corner_state");
    if (!s || !out8) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipMemcpyAsync(out8, s->vi_corner, 8 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_set_corner_state(lb_sim *s, const float *in8)
{
    CPU_UNSUPPORTED(s, "lb_set_corner_state");
    if (s && !s->multifield() && !s->poisson()) SCALAR_UNSUPPORTED(s, "lb_set_corner_state");
    if (!s || !in8) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipMemcpyAsync(s->vi_corner, in8, 8 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_get_feq(lb_sim *s, float *feq)
{
    if (s && s->cpu) {
        if (!feq) return fail(LB_ERR_ARG, "null argument");
        memcpy(feq, s->cpu->feq.data(), sizeof(float) * 9 * s->cpu->plane());     // (as the reference's feq array: whatever update_feq left)
        return LB_OK;
    }
    if (!s || !feq) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc;
    if (!s->feq_valid && (rc = lb_update_feq(s))) return rc;
    const size_t host_plane = (size_t)s->p.nx * s->H;
    for (int k = 0; k < 9; ++k)
        if ((rc = lattice_plane_d2h(s, feq + k * host_plane, s->feq_origin(), k))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_set_mask(lb_sim *s, const int32_t *mask)
{
    if (s && s->cpu) {
        s->cpu->has_mask = mask != nullptr;
        s->cpu->mask.assign(s->cpu->plane(), 0);
        for (size_t c = 0; mask && c < s->cpu->plane(); ++c) s->cpu->mask[c] = mask[c] == 1;
        return LB_OK;
    }
    SCALAR_UNSUPPORTED(s, "lb_set_mask");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    if (!mask) {
        if (s->has_mask && !s->tuned_steps) s->tune_cache_checked = false;     // (another shape as far as LB_TUNE_CACHE is concerned)
        s->has_mask = false;      // (takes effect with the next launch; nothing to upload)
        return LB_OK;
    }
    const size_t n = (size_t)s->pitch * s->H;
    uint8_t *tmp = (uint8_t *)calloc(n, 1);
    if (!tmp) return fail(LB_ERR_ARG, "out of host memory");
    bool any = false;
    for (int y = 0; y < s->H; ++y)
        for (int x = 0; x < s->p.nx; ++x) {
            const uint8_t m = mask[(size_t)y * s->p.nx + x] == 1;   // D2Q9.cl:410 tests == 1
            tmp[(size_t)y * s->pitch + x] = m;
            any |= m;
        }
    // kernels of an un-waited run() may still be reading the mask: the handle's streams are
    // non-blocking, so order the upload behind them explicitly
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->edge_stream);
    if (e == hipSuccess) e = hipMemcpy(s->mask, tmp, n, hipMemcpyHostToDevice);
    free(tmp);
    if (e != hipSuccess) return fail(LB_ERR_HIP, "mask upload: %s", hipGetErrorString(e));
    // An all-zero mask on one slab must still take the MASK kernel if the caller asked for a
    // mask: keep the flag (kernel choice is per handle, results are identical either way).
    (void)any;
    if (!s->has_mask && !s->tuned_steps) s->tune_cache_checked = false;
    s->has_mask = true;
    return LB_OK;
}

int lb_set_mask_halo(lb_sim *s, const int32_t *south_rows, const int32_t *north_rows)
{
    CPU_UNSUPPORTED(s, "lb_set_mask_halo");
    SCALAR_UNSUPPORTED(s, "lb_set_mask_halo");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    uint8_t *tmp = (uint8_t *)calloc((size_t)s->pitch * MASK_GHOST, 1);
    if (!tmp) return fail(LB_ERR_ARG, "out of host memory");
    // south_rows = global rows y0-MASK_GHOST .. y0-1 (nearest last); north_rows = rows y0+H .. y0+H+MASK_GHOST-1
    // (nearest first); each [LB_MASK_HALO_ROWS][nx]
    {
        hipError_t e = hipStreamSynchronize(s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->edge_stream);
        if (e != hipSuccess) {
            free(tmp);
            return fail(LB_ERR_HIP, "mask halo upload: %s", hipGetErrorString(e));
        }
    }
    const int32_t *rows[2] = {south_rows, north_rows};
    uint8_t *dst[2] = {s->mask - (size_t)MASK_GHOST * s->pitch, s->mask + (size_t)s->H * s->pitch};
    for (int side = 0; side < 2; ++side) {
        memset(tmp, 0, (size_t)s->pitch * MASK_GHOST);
        if (rows[side])
            for (int r = 0; r < MASK_GHOST; ++r)
                for (int x = 0; x < s->p.nx; ++x)
                    tmp[(size_t)r * s->pitch + x] = rows[side][(size_t)r * s->p.nx + x] == 1;
        hipError_t e = hipMemcpy(dst[side], tmp, (size_t)s->pitch * MASK_GHOST, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            free(tmp);
            return fail(LB_ERR_HIP, "mask halo upload: %s", hipGetErrorString(e));
        }
    }
    free(tmp);
    return LB_OK;
}

// ---- scalar lattices -----------------------------------------------------------------------
#define NEED_SCALAR(s, name)                                                                                 \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_POROUS(s, name);                                                                                 \
        NOT_ROCKET(s, name);                                                                                 \
        if (!(s)->scalar()) return fail(LB_ERR_STATE, "%s is for scalar lattices (LB_SEM_DIFFUSION)", name); \
    } while (0)

// ... whose velocity is imposed: the Poisson solver has none, and its source term is lb_set_source's
#define NOT_POISSON(s, name)                                                                                 \
    do {                                                                                                     \
        if ((s)->poisson()) return fail(LB_ERR_STATE, "%s is not available on the LB Poisson solver (LB_SEM_POISSON)", name); \
    } while (0)

int lb_set_reaction(lb_sim *s, float G)
{
    NEED_SCALAR(s, "lb_set_reaction");
    NOT_POISSON(s, "lb_set_reaction");
    if (!(fabsf(G) <= 3.0e38f)) return fail(LB_ERR_ARG, "the growth rate must be finite");
    s->ad_G = G;
    return LB_OK;
}

int lb_edge_floats(lb_sim *s)
{
    NEED_SCALAR(s, "lb_edge_floats");
    return (int)edge_host_floats(s);
}

int lb_get_edge_state(lb_sim *s, float *out)
{
    NEED_SCALAR(s, "lb_get_edge_state");
    if (!s->ad_edge) return LB_OK;                  // (PERIODIC: zero floats)
    if (!out) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    const int nx = s->p.nx, ny = s->p.ny;
    const size_t n = (size_t)ad_edge_device_floats(s->pitch, ny);
    float *tmp = (float *)malloc(n * sizeof(float));
    if (!tmp) return fail(LB_ERR_ARG, "out of host memory");
    hipError_t e = hipMemcpyAsync(tmp, s->ad_edge, n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        free(tmp);
        return fail(LB_ERR_HIP, "edge state download: %s", hipGetErrorString(e));
    }
    memcpy(out, tmp + 6 * s->pitch, sizeof(float) * 6 * (size_t)ny);
    float *rows = out + 6 * (size_t)ny;
    for (int r = 0; r < 6; ++r) memcpy(rows + (size_t)r * nx, tmp + (size_t)r * s->pitch, sizeof(float) * (size_t)nx);
    // the four corner links a column and a row share: the column's entry is the one that counts
    rows[1 * (size_t)nx] = out[1 * (size_t)ny];                                 // south f5(0,0) = west f5[0]
    rows[2 * (size_t)nx + nx - 1] = out[4 * (size_t)ny];                        // south f6(nx-1,0) = east f6[0]
    rows[4 * (size_t)nx + nx - 1] = out[5 * (size_t)ny + ny - 1];               // north f7(nx-1,ny-1) = east f7[ny-1]
    rows[5 * (size_t)nx] = out[2 * (size_t)ny + ny - 1];                        // north f8(0,ny-1) = west f8[ny-1]
    free(tmp);
    return LB_OK;
}

int lb_set_edge_state(lb_sim *s, const float *in)
{
    NEED_SCALAR(s, "lb_set_edge_state");
    if (!s->ad_edge) return LB_OK;
    if (!in) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    const int nx = s->p.nx, ny = s->p.ny;
    const size_t n = (size_t)ad_edge_device_floats(s->pitch, ny);
    float *tmp = (float *)calloc(n, sizeof(float));
    if (!tmp) return fail(LB_ERR_ARG, "out of host memory");
    memcpy(tmp + 6 * s->pitch, in, sizeof(float) * 6 * (size_t)ny);
    const float *rows = in + 6 * (size_t)ny;
    for (int r = 0; r < 6; ++r) memcpy(tmp + (size_t)r * s->pitch, rows + (size_t)r * nx, sizeof(float) * (size_t)nx);
    hipError_t e = hipStreamSynchronize(s->stream);       // (kernels of an un-waited run may still be reading it)
    if (e == hipSuccess) e = hipMemcpy(s->ad_edge, tmp, n * sizeof(float), hipMemcpyHostToDevice);
    free(tmp);
    if (e != hipSuccess) return fail(LB_ERR_HIP, "edge state upload: %s", hipGetErrorString(e));
    return LB_OK;
}

int lb_set_velocity_from(lb_sim *s, lb_sim *flow)
{
    NEED_SCALAR(s, "lb_set_velocity_from");
    NOT_POISSON(s, "lb_set_velocity_from");
    if (!flow) return fail(LB_ERR_ARG, "null flow handle");
    if (flow->cpu || flow->scalar() || flow->multi_slab())
        return fail(LB_ERR_ARG, "lb_set_velocity_from takes a whole-grid GPU flow handle");
    if (flow->p.nx != s->p.nx || flow->p.ny != s->p.ny || flow->p.device != s->p.device)
        return fail(LB_ERR_ARG, "the flow handle must have the scalar lattice's grid (%d x %d) and device", s->p.nx, s->p.ny);
    if (flow->stepping) return fail(LB_ERR_STATE, "lb_set_velocity_from inside a split step of the flow handle");
    DeviceGuard guard(s->p.device);
    int rc = ensure_macro(flow);                    // the flow's lazily rebuilt rho, u, v
    if (rc) return rc;
    // on the FLOW handle's stream, behind its work; this handle's kernels may still read u, v, and its later ones must see the new
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));
    HIP_TRY(hipStreamWaitEvent(flow->stream, s->ev_interior, 0));
    // (rho, u, v are [H][pitch] whatever the layout of the lattices: LB_FLAG_PLANAR on either handle does not matter here)
    const long long n4 = s->pitch * s->H / 4;       // (same pitch: same nx)
    for (int i = 0; i < 2; ++i) {
        hipLaunchKernelGGL(k_copy4<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, flow->stream,
                           reinterpret_cast<const f4a *>(i ? flow->v : flow->u), reinterpret_cast<f4a *>(i ? s->v : s->u), n4);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(flow->ev_interior, flow->stream));
    HIP_TRY(hipStreamWaitEvent(s->stream, flow->ev_interior, 0));
    s->feq_valid = false;
    return LB_OK;
}

// ---- the LB Poisson solver ---------------------------------------------------------------------
#define NEED_POISSON(s, name)                                                                                \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_POROUS(s, name);                                                                                 \
        NOT_ROCKET(s, name);                                                                                 \
        if (!(s)->poisson()) return fail(LB_ERR_STATE, "%s is for the LB Poisson solver (LB_SEM_POISSON)", name); \
    } while (0)

// lb_solve's launches between two reads of the stop word.  profiles/poisson_bench.txt: the read-back is one host round trip per batch,
// the launches behind a stop inside a batch are empty early-outs.
static const int PS_BATCH = 32;

int lb_set_poisson(lb_sim *s, float rho_on_boundary, float react_factor, float tolerance)
{
    NEED_POISSON(s, "lb_set_poisson");
    if (!(fabsf(rho_on_boundary) <= 3.0e38f) || !(fabsf(react_factor) <= 3.0e38f)) return fail(LB_ERR_ARG, "rho_on_boundary and react_factor must be finite");
    if (!(tolerance >= 0.f)) return fail(LB_ERR_ARG, "the tolerance must be >= 0");
    s->ps_rho_b = rho_on_boundary;
    s->ps_react = react_factor;
    s->ps_tol = tolerance;
    return LB_OK;
}

int lb_set_source(lb_sim *s, const float *src, int on_device)
{
    NEED_POISSON(s, "lb_set_source");
    if (!src) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipMemcpy2DAsync(s->ps_source, s->pitch * sizeof(float), src, s->p.nx * sizeof(float), s->p.nx * sizeof(float), s->H,
                             on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_get_source(lb_sim *s, float *src)
{
    NEED_POISSON(s, "lb_get_source");
    if (!src) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc = copy_plane_d2h(s, src, s->ps_source);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_solve_reset(lb_sim *s)
{
    NEED_POISSON(s, "lb_solve_reset");
    s->ps_iter = 0;
    return LB_OK;
}

int lb_get_solve_state(lb_sim *s, int *iterations, int *stop_word)
{
    NEED_POISSON(s, "lb_get_solve_state");
    DeviceGuard guard(s->p.device);
    PsState h;
    HIP_TRY(hipMemcpyAsync(&h, s->ps_state, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (iterations) *iterations = s->ps_iter;
    if (stop_word) *stop_word = h.stop;
    return LB_OK;
}

int lb_set_solve_state(lb_sim *s, int iterations, int stop_word)
{
    NEED_POISSON(s, "lb_set_solve_state");
    if (iterations < 0 || stop_word < 0 || stop_word > iterations) return fail(LB_ERR_ARG, "need 0 <= stop_word <= iterations");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(&s->ps_state->stop, &stop_word, sizeof(int), hipMemcpyHostToDevice));
    s->ps_iter = iterations;
    return LB_OK;
}

// solver.py:324-358 without its host waits: per iteration one k_ps_step<true> and -- from the second iteration since the last reset --
// one k_ps_check, PS_BATCH iterations enqueued at a time; after each batch the stop word comes back (4 bytes).  A stop at iteration
// n* leaves the launches behind it as empty early-outs, so the populations and rho are those after n* iterations; which lattice of the
// pair holds them follows from n*.
int lb_solve(lb_sim *s, int max_iterations, int *iterations_done, int *converged, float *last_ratio)
{
    NEED_POISSON(s, "lb_solve");
    if (max_iterations < 0) return fail(LB_ERR_ARG, "negative iteration count");
    DeviceGuard guard(s->p.device);
    const int batch = s->ps_batch > 0 ? s->ps_batch : PS_BATCH, first = s->ps_iter, cur0 = s->cur;
    const long long blocks = ps_step_blocks(step_args(s, 0, 1, s->H));
    const PsExtra e = ps_extra(s);
    HIP_TRY(hipMemsetAsync(&s->ps_state->stop, 0, sizeof(int), s->stream));     // (a call after a stop goes on, as the reference's run does)
    int launched = 0, stop = 0;
    while (launched < max_iterations && !stop) {
        const int nb = std::min(batch, max_iterations - launched);
        for (int i = 0; i < nb; ++i, ++launched) {
            const int it = first + launched + 1;
            lbk_ps_step(true, s->stream, step_args(s, 0, 1, s->H), e);
            HIP_TRY(hipGetLastError());
            s->cur ^= 1;
            if (it >= 2) {
                lbk_ps_check(s->stream, s->ps_part, blocks, s->ps_state, it, s->ps_tol);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipMemcpyAsync(&stop, &s->ps_state->stop, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    const int done = stop ? stop - first : launched;
    s->cur = cur0 ^ (done & 1);
    s->ps_iter = first + done;
    if (done) { s->feq_valid = false; s->macro_valid = true; }
    if (last_ratio) {
        HIP_TRY(hipMemcpyAsync(last_ratio, &s->ps_state->ratio, sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (iterations_done) *iterations_done = done;
    if (converged) *converged = stop ? 1 : 0;
    return LB_OK;
}

// One launch into the handle's u, v planes -- which no other kernel of this semantics writes: they hold the last gradient, lb_get_macro
// returns it --, then one pitched copy each to wherever the caller's pointers lead.
int lb_gradient(lb_sim *s, float inv_two_dx, float *ddx, float *ddy)
{
    NEED_POISSON(s, "lb_gradient");
    if (!(fabsf(inv_two_dx) <= 3.0e38f)) return fail(LB_ERR_ARG, "inv_two_dx must be finite");
    DeviceGuard guard(s->p.device);
    lbk_ps_gradient(s->stream, step_args(s, 0, 1, s->H), inv_two_dx);
    HIP_TRY(hipGetLastError());
    float *out[2] = {ddx, ddy};
    const float *from[2] = {s->u, s->v};
    for (int i = 0; i < 2; ++i)
        if (out[i])
            HIP_TRY(hipMemcpy2DAsync(out[i], s->p.nx * sizeof(float), from[i], s->pitch * sizeof(float), s->p.nx * sizeof(float), s->H,
                                     hipMemcpyDefault, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

// ---- forced flow in a porous medium ------------------------------------------------------------
#define NEED_POROUS(s, name)                                                                                 \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_ROCKET(s, name);                                                                                 \
        if ((s)->multifluid()) return fail(LB_ERR_STATE, "%s is not available on a fluid of a multicomponent set (LB_SEM_MULTIFLUID)", name); \
        if (!(s)->porous()) return fail(LB_ERR_STATE, "%s is for forced flow in a porous medium (LB_SEM_POROUS)", name); \
    } while (0)
// (the calls a fluid of a multicomponent set shares with the porous-medium fluid: its g, its force field, G and u_b)
#define NEED_FORCED(s, name)                                                                                 \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_ROCKET(s, name);                                                                                 \
        if (!(s)->porous() && !(s)->multifluid())                                                            \
            return fail(LB_ERR_STATE, "%s is for forced flow in a porous medium (LB_SEM_POROUS) and the fluids of a multicomponent set (LB_SEM_MULTIFLUID)", name); \
    } while (0)

static bool pm_finite(float x) { return fabsf(x) <= 3.0e38f; }      // (false for NaN)

int lb_set_porous(lb_sim *s, float epsilon, float nu_fluid, float K, float Fe)
{
    NEED_POROUS(s, "lb_set_porous");
    if (!pm_finite(epsilon) || !pm_finite(nu_fluid) || !pm_finite(K) || !pm_finite(Fe)) return fail(LB_ERR_ARG, "epsilon, nu_fluid, K and Fe must be finite");
    if (!(epsilon > 0.f) || !(K > 0.f)) return fail(LB_ERR_ARG, "need epsilon > 0 and K > 0 (got %g, %g)", epsilon, K);
    s->pm_eps = epsilon; s->pm_nu = nu_fluid; s->pm_K = K; s->pm_Fe = Fe;
    s->feq_valid = false;
    return LB_OK;
}

int lb_set_body_force(lb_sim *s, float gx, float gy)
{
    NEED_FORCED(s, "lb_set_body_force");
    if (!pm_finite(gx) || !pm_finite(gy)) return fail(LB_ERR_ARG, "the body force must be finite");
    s->pm_gx = gx; s->pm_gy = gy;
    return LB_OK;
}

int lb_set_force_field(lb_sim *s, const float *gx, const float *gy, int on_device)
{
    NEED_FORCED(s, "lb_set_force_field");
    if ((gx == nullptr) != (gy == nullptr)) return fail(LB_ERR_ARG, "both planes of the force field, or neither");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));       // (kernels of an un-waited run may still be reading it)
    if (!gx) {
        for (float *&q : s->pm_field) {
            if (q) {
                HIP_TRY(hipFree(q));
                s->bytes -= (int64_t)sizeof(float) * s->pitch * s->H;
            }
            q = nullptr;
        }
        s->has_field = false;
        return LB_OK;
    }
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    const float *from[2] = {gx, gy};
    for (int i = 0; i < 2; ++i) {
        if (!s->pm_field[i]) {
            HIP_TRY(hipMalloc(&s->pm_field[i], fld_bytes));
            s->bytes += (int64_t)fld_bytes;
        }
        HIP_TRY(hipMemsetAsync(s->pm_field[i], 0, fld_bytes, s->stream));
        HIP_TRY(hipMemcpy2DAsync(s->pm_field[i], s->pitch * sizeof(float), from[i], s->p.nx * sizeof(float), s->p.nx * sizeof(float), s->H,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_field = true;
    return LB_OK;
}

static int pm_get_pair(lb_sim *s, float *const (&pair)[2], float *a, float *b)
{
    DeviceGuard guard(s->p.device);
    int rc;
    if (a && (rc = copy_plane_d2h(s, a, pair[0]))) return rc;
    if (b && (rc = copy_plane_d2h(s, b, pair[1]))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_get_force(lb_sim *s, float *Gx, float *Gy)
{
    NEED_FORCED(s, "lb_get_force");
    return pm_get_pair(s, s->pm_G, Gx, Gy);
}

int lb_get_bary_velocity(lb_sim *s, float *u_bary, float *v_bary)
{
    NEED_FORCED(s, "lb_get_bary_velocity");
    return pm_get_pair(s, s->pm_ub, u_bary, v_bary);
}

int lb_set_bary_velocity(lb_sim *s, const float *u_bary, const float *v_bary)
{
    NEED_FORCED(s, "lb_set_bary_velocity");
    if (!u_bary || !v_bary) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc;
    if ((rc = copy_plane_h2d(s, s->pm_ub[0], u_bary))) return rc;
    if ((rc = copy_plane_h2d(s, s->pm_ub[1], v_bary))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->feq_valid = false;
    return LB_OK;
}

// (checkpoints: the total force as the last step left it)
int lb_set_force(lb_sim *s, const float *Gx, const float *Gy)
{
    NEED_FORCED(s, "lb_set_force");
    if (!Gx || !Gy) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    int rc;
    if ((rc = copy_plane_h2d(s, s->pm_G[0], Gx))) return rc;
    if ((rc = copy_plane_h2d(s, s->pm_G[1], Gy))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_update_forces(lb_sim *s)
{
    NEED_FORCED(s, "lb_update_forces");
    if (s->multifluid()) return lb_update_forces_fluids(&s, 1);
    DeviceGuard guard(s->p.device);
    lbk_pm_forces(s->stream, step_args(s, 0, 1, s->H), pm_extra(s));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int lb_update_bary_velocity(lb_sim *s)
{
    NEED_FORCED(s, "lb_update_bary_velocity");
    if (s->multifluid()) return lb_update_bary_fluids(&s, 1);
    DeviceGuard guard(s->p.device);
    lbk_pm_bary(s->stream, step_args(s, 0, 1, s->H), pm_extra(s), s->origin(s->cur));
    HIP_TRY(hipGetLastError());
    s->feq_valid = false;
    return LB_OK;
}

// ---- un-fused phases ---------------------------------------------------------------------

int lb_move(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->move(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_move");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    if ((rc = ensure_macro(s))) return rc;
    if (s->p.semantics == LB_SEM_CYTHON) {
        // every entry of the target is written, so the lattices simply swap
        hipLaunchKernelGGL(k1_move, cells_grid(s, 9), dim3(256), 0, s->stream, phase_args(s));
        HIP_TRY(hipGetLastError());
        s->cur ^= 1;
        return LB_OK;
    }
    hipLaunchKernelGGL(k_move, cells_grid(s, 9), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    // copy_buffer: f = f_streamed (kept as a copy, not a pointer swap, so that the stale
    // never-written entries of f_streamed behave exactly like the reference's)
    {
        int rc = copy_lattice(s, s->lat[s->cur], s->lat[s->cur ^ 1]);
        if (rc) return rc;
    }
    return frozen_patch(s, s->cur);
}

int lb_move_bcs(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->move_bcs(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_move_bcs");
    if (rc) return rc;
    if (s->scalar() && s->p.bc_mode != LB_BC_BOX && !s->poisson()) return LB_OK;     // (diffusion.py:326-331: `pass`; the periodic families have none)
    if ((s->porous() || s->multifluid()) && s->p.bc_mode == LB_BC_PERIODIC) return LB_OK;                 // (single_component.py:155-156: `pass`)
    DeviceGuard guard(s->p.device);
    if (s->porous() || s->multifluid()) {           // single_component.cl's and multi.cl's move_open_bcs: boundary cells copy their interior neighbour
        lbk_pm_move_bcs(s->stream, step_args(s, 0, 1, s->H), s->origin(s->cur));
        HIP_TRY(hipGetLastError());
        return LB_OK;
    }
    if (s->poisson()) {                             // D2Q9_poisson.cl's move_bcs: the prescribed value on four walls
        lbk_ps_move_bcs(s->stream, step_args(s, 0, 1, s->H), s->origin(s->cur), ps_extra(s).wall);
        HIP_TRY(hipGetLastError());
        return LB_OK;
    }
    if (s->scalar()) {                              // D2Q9_multifield_fisher.cl's move_bcs: on-node bounce-back on four walls
        lbk_mf_move_bcs(s->stream, step_args(s, 0, 1, s->H), s->origin(s->cur));
        HIP_TRY(hipGetLastError());
        return LB_OK;
    }
    if ((rc = ensure_macro(s))) return rc;
    if (s->p.semantics == LB_SEM_CYTHON)
        hipLaunchKernelGGL(k1_bcs, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    else if (s->p.bc_mode == LB_BC_VELOCITY_INLET) {
        hipLaunchKernelGGL(k_bcs_vel, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
        HIP_TRY(hipGetLastError());
        if (s->has_mask) hipLaunchKernelGGL(k_bounce, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    } else
        hipLaunchKernelGGL(k_bcs, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int lb_update_hydro(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->update_hydro(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_update_hydro");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    if (s->multifluid())
        lbk_mc_hydro(s->stream, step_args(s, 0, 1, s->H));       // rho, and u, v where rho > 1e-12
    else if (s->porous())
        lbk_pm_hydro(s->stream, step_args(s, 0, 1, s->H));       // rho, and u, v where rho > 1e-6
    else if (s->poisson())
        lbk_ps_hydro(s->stream, step_args(s, 0, 1, s->H));       // rho = (9/5)(f1 + ... + f8)
    else if (s->scalar())
        lbk_ad_hydro(s->stream, step_args(s, 0, 1, s->H));       // rho only: u, v are imposed
    else if (s->p.semantics == LB_SEM_CYTHON)
        hipLaunchKernelGGL(k1_hydro, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    else if (s->p.bc_mode == LB_BC_VELOCITY_INLET)
        hipLaunchKernelGGL(k_hydro_vel, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    else if (s->p.semantics == LB_SEM_OPENCL_D2Q9I) {
        // D2Q9i.cl:67-97 + the cylinder class's override (opencl_dim_D2Q9i.py:494-503): u, v zeroed in the obstacle
        hipLaunchKernelGGL(k_hydro_i, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
        HIP_TRY(hipGetLastError());
        if (s->has_mask) hipLaunchKernelGGL(k_zero_vel, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    } else
        hipLaunchKernelGGL(k_hydro, cells_grid(s, 1), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    s->macro_valid = true;
    return LB_OK;   // feq keeps its previous content, as the reference's feq buffer does
}

int lb_update_feq(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->update_feq(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    int rc = ensure_feq(s);
    if (rc) return rc;
    if ((rc = ensure_macro(s))) return rc;
    PhaseArgs a = phase_args(s);
    a.ny = s->H;   // rho,u,v are local: valid for slabs too
    if (s->porous() || s->multifluid())
        lbk_pm_feq(s->stream, step_args(s, 0, 1, s->H), pm_extra(s), s->feq_origin());      // from rho and u_b (a fluid of a multicomponent set: epsilon = 1)
    else if (s->poisson())
        lbk_ps_feq(s->stream, step_args(s, 0, 1, s->H), s->feq_origin());
    else if (s->scalar())
        lbk_ad_feq(s->stream, step_args(s, 0, 1, s->H), s->feq_origin());
    else if (s->p.semantics == LB_SEM_OPENCL_D2Q9I)
        hipLaunchKernelGGL(k_feq_i, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    else
        hipLaunchKernelGGL(k_feq, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    s->feq_valid = true;
    return LB_OK;
}

int lb_collide_particles(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->collide(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_collide_particles");
    if (rc) return rc;
    NOT_ROCKET(s, "lb_collide_particles (the collision needs both members: lb_collide_rocket)");
    if (!s->feq) return fail(LB_ERR_STATE, "lb_collide_particles before any lb_update_feq");
    if (s->multifield()) return lb_collide_coupled(&s, 1);
    DeviceGuard guard(s->p.device);
    if ((rc = ensure_macro(s))) return rc;
    if (s->multifluid())
        lbk_mc_relax(s->stream, step_args(s, 0, 1, s->H), pm_extra(s), s->origin(s->cur), s->feq_origin());
    else if (s->porous())
        lbk_pm_collide(s->stream, step_args(s, 0, 1, s->H), pm_extra(s), s->origin(s->cur), s->feq_origin());
    else if (s->poisson())
        lbk_ps_collide(s->stream, step_args(s, 0, 1, s->H), s->origin(s->cur), s->feq_origin(), s->ps_source, s->ps_react);
    else if (s->scalar())
        lbk_ad_collide(s->ad_G != 0.f, s->stream, step_args(s, 0, 1, s->H), s->origin(s->cur), s->feq_origin(), s->ad_G);
    else
        hipLaunchKernelGGL(k_collide, cells_grid(s, 9), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int lb_zero_velocity_in_obstacle(lb_sim *s)
{
    if (s && s->cpu) {
        for (size_t c = 0; s->cpu->has_mask && c < s->cpu->plane(); ++c)
            if (s->cpu->mask[c]) { s->cpu->u[c] = 0.; s->cpu->v[c] = 0.; }
        return LB_OK;
    }
    SCALAR_UNSUPPORTED(s, "lb_zero_velocity_in_obstacle");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (!s->has_mask) return LB_OK;
    DeviceGuard guard(s->p.device);
    {
        int rc = ensure_macro(s);
        if (rc) return rc;
    }
    PhaseArgs a = phase_args(s);
    hipLaunchKernelGGL(k_zero_vel, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int lb_init_pop(lb_sim *s)
{
    if (s && s->cpu) {                               // f = feq (cython_dim.pyx:191-197; the perturbation is the host class's)
        s->cpu->f = s->cpu->feq;
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    int rc;
    if (!s->feq_valid && (rc = lb_update_feq(s))) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = copy_lattice(s, s->lat[i], s->feq))) return rc;
    s->ghost_depth = 0;
    return frozen_capture(s, s->cur);
}

// ---- fused stepping (lb_step_*, lb_halo_*, lb_run_group: slab.cpp) --------------------------
int lb_run(lb_sim *s, int n_steps)
{
    if (s && s->cpu) {
        if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
        s->cpu->run(n_steps);
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_run between lb_step_boundary and lb_step_finish");
    NOT_ROCKET(s, "lb_run (a colony advances as a set of two: lb_run_rocket)");
    DeviceGuard guard(s->p.device);
    if (s->multifield()) return lb_run_coupled(&s, 1, n_steps);
    if (s->poisson()) return run_poisson(s, n_steps);
    if (s->porous()) return run_porous(s, n_steps);
    if (s->multifluid()) return lb_run_fluids(&s, 1, n_steps);
    if (s->scalar()) return run_scalar(s, n_steps);
    if (!s->tune_cache_checked) (void)tune_cache_apply(s);
    if (s->p.semantics == LB_SEM_CYTHON) return run_cython(s, n_steps);
    if (!s->multi_slab()) return run_whole_grid(s, n_steps);     // (never blocks the host: tuning is lb_autotune*'s job)
    return run_slab(s, n_steps);
}

// Population sets: `count` periodic whole-grid lattices of one geometry (one per population of a multi-population
// model, each with its own omega / mask content) advanced in lock step, ONE launch per time step for all of them.
int lb_run_batch(lb_sim **sims, int count, int n_steps)
{
    for (int i = 0; sims && i < count; ++i) CPU_UNSUPPORTED(sims[i], "lb_run_batch");
    for (int i = 0; sims && i < count; ++i) SCALAR_UNSUPPORTED(sims[i], "lb_run_batch");
    if (!sims || count < 1 || count > BATCH_MAX || n_steps < 0)
        return fail(LB_ERR_ARG, "lb_run_batch takes 1..%d handles and a non-negative step count", BATCH_MAX);
    for (int i = 0; i < count; ++i) {
        lb_sim *s = sims[i];
        if (!s) return fail(LB_ERR_ARG, "null handle in batch");
        if (s->multi_slab() || s->p.bc_mode != LB_BC_PERIODIC || s->p.semantics != LB_SEM_OPENCL)
            return fail(LB_ERR_ARG, "batch members must be whole-grid periodic OpenCL-path handles");
        if (s->p.nx != sims[0]->p.nx || s->p.ny != sims[0]->p.ny || s->p.device != sims[0]->p.device ||
            s->has_mask != sims[0]->has_mask)
            return fail(LB_ERR_ARG, "batch members must share grid, device and obstacle-mask presence");
        if (s->stepping) return fail(LB_ERR_STATE, "lb_run_batch inside a split step");
        for (int j = 0; j < i; ++j)
            if (sims[j] == s) return fail(LB_ERR_ARG, "a handle appears twice in the batch");
    }
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = sims[0];
    DeviceGuard guard(s0->p.device);
    // everything is enqueued on the first member's stream, behind whatever the others still have in flight
    for (int i = 1; i < count; ++i) {
        HIP_TRY(hipEventRecord(sims[i]->ev_interior, sims[i]->stream));
        HIP_TRY(hipStreamWaitEvent(s0->stream, sims[i]->ev_interior, 0));
    }
    const dim3 block(256, 1);
    const dim3 grid((unsigned)((s0->pitch / 4 + 255) / 256), (unsigned)s0->H, (unsigned)count);
    bool lazy = true;              // (one launch serves all members: rho, u, v are stored unless every member rebuilds them on demand)
    for (int i = 0; i < count; ++i) lazy = lazy && lazy_macro(sims[i]);
    for (int it = 0; it < n_steps; ++it) {
        BatchArgs b;
        for (int i = 0; i < count; ++i) b.a[i] = step_args(sims[i], 0, 1, sims[i]->H);
        const bool macro = (it == n_steps - 1) && !lazy;
        lbk_launch_step_batch(s0->has_mask, macro, grid, block, s0->stream, b);
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < count; ++i) sims[i]->cur ^= 1;
    }
    // the other members' streams see the result
    HIP_TRY(hipEventRecord(s0->ev_interior, s0->stream));
    for (int i = 0; i < count; ++i) {
        if (i) HIP_TRY(hipStreamWaitEvent(sims[i]->stream, s0->ev_interior, 0));
        sims[i]->feq_valid = false;
        sims[i]->macro_valid = !lazy;
    }
    return LB_OK;
}

// Coupled scalar lattices: the members of a set, checked alike for lb_run_coupled and lb_collide_coupled.
static int coupled_members(lb_sim **f, int count, const char *what)
{
    if (!f || count < 1 || count > MF_MAX) return fail(LB_ERR_ARG, "%s takes 1..%d handles", what, MF_MAX);
    for (int i = 0; i < count; ++i) {
        lb_sim *s = f[i];
        if (!s) return fail(LB_ERR_ARG, "null handle in the coupled set");
        if (s->cpu || !s->multifield()) return fail(LB_ERR_ARG, "the members of a coupled set must be LB_SEM_MULTIFIELD handles");
        if (s->p.nx != f[0]->p.nx || s->p.ny != f[0]->p.ny || s->p.bc_mode != f[0]->p.bc_mode || s->p.device != f[0]->p.device ||
            (s->p.flags & LB_FLAG_PLANAR) != (f[0]->p.flags & LB_FLAG_PLANAR))
            return fail(LB_ERR_ARG, "the members of a coupled set must share grid, boundary family, layout flag and device");
        if (s->stepping) return fail(LB_ERR_STATE, "%s inside a split step", what);
        for (int j = 0; j < i; ++j)
            if (f[j] == s) return fail(LB_ERR_ARG, "a handle appears twice in the coupled set");
    }
    return LB_OK;
}

// everything of a coupled call is enqueued on the first member's stream, behind whatever the others still have in flight ...
static int coupled_join(lb_sim **f, int count)
{
    for (int i = 1; i < count; ++i) {
        HIP_TRY(hipEventRecord(f[i]->ev_interior, f[i]->stream));
        HIP_TRY(hipStreamWaitEvent(f[0]->stream, f[i]->ev_interior, 0));
    }
    return LB_OK;
}
// ... and the other members' streams see the result
static int coupled_release(lb_sim **f, int count)
{
    if (count < 2) return LB_OK;
    HIP_TRY(hipEventRecord(f[0]->ev_interior, f[0]->stream));
    for (int i = 1; i < count; ++i) HIP_TRY(hipStreamWaitEvent(f[i]->stream, f[0]->ev_interior, 0));
    return LB_OK;
}

int lb_run_coupled(lb_sim **fields, int count, int n_steps)
{
    for (int i = 0; fields && i < count; ++i) NOT_POROUS(fields[i], "lb_run_coupled");
    for (int i = 0; fields && i < count; ++i) NOT_ROCKET(fields[i], "lb_run_coupled");
    int rc = coupled_members(fields, count, "lb_run_coupled");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fields[0];
    DeviceGuard guard(s0->p.device);
    if ((rc = coupled_join(fields, count))) return rc;
    for (int it = 0; it < n_steps; ++it) {
        MfArgs m = {};
        for (int i = 0; i < count; ++i) {
            m.a[i] = step_args(fields[i], 0, 1, fields[i]->H);
            m.G[i] = fields[i]->ad_G;
        }
        lbk_mf_step(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);      // the last launch stores every field's rho
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < count; ++i) fields[i]->cur ^= 1;
    }
    for (int i = 0; i < count; ++i) {
        fields[i]->feq_valid = false;
        fields[i]->macro_valid = true;
    }
    return coupled_release(fields, count);
}

int lb_collide_coupled(lb_sim **fields, int count)
{
    int rc = coupled_members(fields, count, "lb_collide_coupled");
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_coupled before lb_update_feq on every member");
    lb_sim *s0 = fields[0];
    DeviceGuard guard(s0->p.device);
    if ((rc = coupled_join(fields, count))) return rc;
    MfArgs m = {};
    for (int i = 0; i < count; ++i) {
        m.a[i] = step_args(fields[i], 0, 1, fields[i]->H);
        m.a[i].dst = fields[i]->origin(fields[i]->cur);         // relaxed in place
        m.G[i] = fields[i]->ad_G;
        m.feq[i] = fields[i]->feq_origin();
    }
    lbk_mf_collide(count, s0->stream, m);
    HIP_TRY(hipGetLastError());
    return coupled_release(fields, count);
}

// ---- multicomponent Shan-Chen fluids: the members of a set, checked alike for every set call ---------------------------------
static int fluid_members(lb_sim **f, int count, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count < 1 || count > MC_MAX) return fail(LB_ERR_ARG, "%s takes 1..%d handles (more than %d fluids are not built)", what, MC_MAX, MC_MAX);
    for (int i = 0; i < count; ++i) {
        lb_sim *s = f[i];
        if (!s) return fail(LB_ERR_ARG, "null handle in the set of fluids");
        NOT_ROCKET(s, what);
        if (s->cpu || !s->multifluid()) return fail(LB_ERR_STATE, "%s is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)", what);
        if (s->p.nx != f[0]->p.nx || s->p.ny != f[0]->p.ny || s->p.bc_mode != f[0]->p.bc_mode || s->p.device != f[0]->p.device ||
            (s->p.flags & LB_FLAG_PLANAR) != (f[0]->p.flags & LB_FLAG_PLANAR))
            return fail(LB_ERR_ARG, "the fluids of a set must share grid, boundary family, layout flag and device (fluids of different families in one set are not built)");
        for (int j = 0; j < i; ++j)
            if (f[j] == s) return fail(LB_ERR_ARG, "a handle appears twice in the set of fluids");
    }
    // the tables name fluids by their place in the set
    for (int t = 0; t < f[0]->mc_n_inter; ++t)
        if (f[0]->mc_inter[t].i >= count || f[0]->mc_inter[t].j >= count)
            return fail(LB_ERR_STATE, "%s: the interaction table of the first handle names fluid %d of a set of %d", what,
                        f[0]->mc_inter[t].i > f[0]->mc_inter[t].j ? f[0]->mc_inter[t].i : f[0]->mc_inter[t].j, count);
    for (int t = 0; t < f[0]->mc_n_react; ++t)
        if (f[0]->mc_react[t].a >= count || f[0]->mc_react[t].b >= count)
            return fail(LB_ERR_STATE, "%s: the reaction table of the first handle names a fluid outside a set of %d", what, count);
    return LB_OK;
}

// (src = dst = the current lattice: what the phases read and write in place; the two-launch step sets dst itself)
static McArgs fluid_args(lb_sim **f, int count)
{
    McArgs m = {};
    for (int i = 0; i < count; ++i) {
        m.a[i] = step_args(f[i], 0, 1, f[i]->H);
        m.e[i] = pm_extra(f[i]);
    }
    for (int t = 0; t < f[0]->mc_n_inter; ++t) m.inter[t] = f[0]->mc_inter[t];
    for (int t = 0; t < f[0]->mc_n_react; ++t) m.react[t] = f[0]->mc_react[t];
    m.n_inter = f[0]->mc_n_inter;
    m.n_react = f[0]->mc_n_react;
    return m;
}

int lb_run_fluids(lb_sim **fluids, int count, int n_steps)
{
    int rc = fluid_members(fluids, count, "lb_run_fluids");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fluids[0];
    DeviceGuard guard(s0->p.device);
    if ((rc = coupled_join(fluids, count))) return rc;
    for (int it = 0; it < n_steps; ++it) {
        const McArgs m = fluid_args(fluids, count);
        if (multifluid_one_launch(s0)) {            // (the set's first handle chooses: lb_set_variant; plan.cpp)
            lbk_mc_step(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);        // the last one stores rho, u, v, G and u_b
            HIP_TRY(hipGetLastError());
        } else {
            lbk_mc_moments(s0->p.bc_mode, count, s0->stream, m);
            HIP_TRY(hipGetLastError());
            lbk_mc_collide(s0->p.bc_mode, count, it == n_steps - 1, s0->stream, m);     // the last one stores u, v, G and u_b
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < count; ++i) fluids[i]->cur ^= 1;
    }
    for (int i = 0; i < count; ++i) {
        fluids[i]->feq_valid = false;
        fluids[i]->macro_valid = true;
    }
    return coupled_release(fluids, count);
}

static bool mc_finite(float x) { return fabsf(x) <= 3.0e38f; }      // (false for NaN)

int lb_set_interactions(lb_sim **fluids, int count, const lb_interaction *table, int n)
{
    int rc = fluid_members(fluids, count, "lb_set_interactions");
    if (rc) return rc;
    if (n < 0 || n > MC_MAX_INTER || (n > 0 && !table)) return fail(LB_ERR_ARG, "lb_set_interactions takes 0..%d entries", MC_MAX_INTER);
    McInter in[MC_MAX_INTER] = {};
    for (int t = 0; t < n; ++t) {
        const lb_interaction &e = table[t];
        if (e.fluid_1 < 0 || e.fluid_1 >= count || e.fluid_2 < 0 || e.fluid_2 >= count)
            return fail(LB_ERR_ARG, "interaction %d names fluids %d and %d of a set of %d", t, e.fluid_1, e.fluid_2, count);
        if (e.potential != LB_PSI_LINEAR && e.potential != LB_PSI_SHAN_CHEN && e.potential != LB_PSI_POW)
            return fail(LB_ERR_ARG, "interaction %d: unknown potential %d (linear, shan_chen and pow are built; vdw is not)", t, e.potential);
        if (e.boundary != (fluids[0]->p.bc_mode == LB_BC_PERIODIC ? 0 : 1))
            return fail(LB_ERR_ARG, "interaction %d: the stencil's boundary rule (%d) must be the set's family (%s)", t, e.boundary,
                        fluids[0]->p.bc_mode == LB_BC_PERIODIC ? "0, periodic" : "1, zero gradient");
        if (!mc_finite(e.G_int) || !mc_finite(e.parameter)) return fail(LB_ERR_ARG, "interaction %d: G_int and the parameter must be finite", t);
        if (e.potential == LB_PSI_SHAN_CHEN && e.parameter == 0.f) return fail(LB_ERR_ARG, "interaction %d: shan_chen needs rho_0 != 0", t);
        in[t] = McInter{e.fluid_1, e.fluid_2, e.potential, e.G_int, e.parameter};
    }
    for (int t = 0; t < MC_MAX_INTER; ++t) fluids[0]->mc_inter[t] = in[t];
    fluids[0]->mc_n_inter = n;
    return LB_OK;
}

int lb_set_reactions(lb_sim **fluids, int count, const lb_fluid_reaction *table, int n)
{
    int rc = fluid_members(fluids, count, "lb_set_reactions");
    if (rc) return rc;
    if (n < 0 || n > MC_MAX_REACT || (n > 0 && !table)) return fail(LB_ERR_ARG, "lb_set_reactions takes 0..%d entries", MC_MAX_REACT);
    McReact re[MC_MAX_REACT] = {};
    for (int t = 0; t < n; ++t) {
        const lb_fluid_reaction &e = table[t];
        if (e.kind != LB_REACT_EAT && e.kind != LB_REACT_GROW) return fail(LB_ERR_ARG, "reaction %d: unknown kind %d", t, e.kind);
        if (e.fluid_a < 0 || e.fluid_a >= count) return fail(LB_ERR_ARG, "reaction %d names fluid %d of a set of %d", t, e.fluid_a, count);
        if (e.kind == LB_REACT_EAT && (e.fluid_b < 0 || e.fluid_b >= count || e.fluid_b == e.fluid_a))
            return fail(LB_ERR_ARG, "reaction %d: the eatee must be another fluid of the set (got %d, eater %d)", t, e.fluid_b, e.fluid_a);
        if (!mc_finite(e.p0) || !mc_finite(e.p1) || !mc_finite(e.p2)) return fail(LB_ERR_ARG, "reaction %d: the parameters must be finite", t);
        re[t] = McReact{e.kind, e.fluid_a, e.kind == LB_REACT_EAT ? e.fluid_b : 0, e.p0, e.p1, e.p2};
    }
    for (int t = 0; t < MC_MAX_REACT; ++t) fluids[0]->mc_react[t] = re[t];
    fluids[0]->mc_n_react = n;
    return LB_OK;
}

int lb_get_interactions(lb_sim *first, lb_interaction *table, int *n)
{
    if (!first) return fail(LB_ERR_ARG, "null handle");
    NOT_ROCKET(first, "lb_get_interactions");
    if (first->cpu || !first->multifluid()) return fail(LB_ERR_STATE, "lb_get_interactions is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)");
    if (n) *n = first->mc_n_inter;
    for (int t = 0; table && t < first->mc_n_inter; ++t) {
        const McInter &e = first->mc_inter[t];
        table[t] = lb_interaction{e.i, e.j, e.potential, first->p.bc_mode == LB_BC_PERIODIC ? 0 : 1, e.G, e.par};
    }
    return LB_OK;
}

int lb_get_reactions(lb_sim *first, lb_fluid_reaction *table, int *n)
{
    if (!first) return fail(LB_ERR_ARG, "null handle");
    NOT_ROCKET(first, "lb_get_reactions");
    if (first->cpu || !first->multifluid()) return fail(LB_ERR_STATE, "lb_get_reactions is for the fluids of a multicomponent set (LB_SEM_MULTIFLUID)");
    if (n) *n = first->mc_n_react;
    for (int t = 0; table && t < first->mc_n_react; ++t) {
        const McReact &e = first->mc_react[t];
        table[t] = lb_fluid_reaction{e.kind, e.a, e.b, e.p0, e.p1, e.p2};
    }
    return LB_OK;
}

int lb_update_forces_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_update_forces_fluids");
    if (rc) return rc;
    DeviceGuard guard(fluids[0]->p.device);
    if ((rc = coupled_join(fluids, count))) return rc;
    lbk_mc_forces(fluids[0]->p.bc_mode, count, fluids[0]->stream, fluid_args(fluids, count));
    HIP_TRY(hipGetLastError());
    return coupled_release(fluids, count);
}

int lb_update_bary_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_update_bary_fluids");
    if (rc) return rc;
    DeviceGuard guard(fluids[0]->p.device);
    if ((rc = coupled_join(fluids, count))) return rc;
    lbk_mc_bary(count, fluids[0]->stream, fluid_args(fluids, count));
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < count; ++i) fluids[i]->feq_valid = false;
    return coupled_release(fluids, count);
}

int lb_react_fluids(lb_sim **fluids, int count)
{
    int rc = fluid_members(fluids, count, "lb_react_fluids");
    if (rc) return rc;
    if (fluids[0]->mc_n_react == 0) return LB_OK;
    DeviceGuard guard(fluids[0]->p.device);
    if ((rc = coupled_join(fluids, count))) return rc;
    McArgs m = fluid_args(fluids, count);
    for (int i = 0; i < count; ++i) m.a[i].dst = fluids[i]->origin(fluids[i]->cur);       // in place
    lbk_mc_react(count, fluids[0]->stream, m);
    HIP_TRY(hipGetLastError());
    return coupled_release(fluids, count);
}

// ---- surfactant-propelled colonies: the two members of a set, checked alike for every set call -----------------------------------
static int rocket_members(lb_sim **f, int count, const char *what)
{
    if (!f) return fail(LB_ERR_ARG, "%s: null handle array", what);
    if (count != 2) return fail(LB_ERR_ARG, "%s takes exactly 2 handles, the population and the surfactant (got a count of %d)", what, count);
    for (int i = 0; i < 2; ++i) {
        lb_sim *s = f[i];
        if (!s) return fail(LB_ERR_ARG, "%s: null handle in the set", what);
        if (s->cpu || !s->rocket()) return fail(LB_ERR_ARG, "%s: handle %d is not a lattice of a surfactant-propelled colony (a non-rocket handle: LB_SEM_ROCKET is required)", what, i);
        if (s->stepping) return fail(LB_ERR_STATE, "%s inside a split step", what);
    }
    if (f[0] == f[1]) return fail(LB_ERR_ARG, "%s: a handle appears twice in the set", what);
    if (f[1]->p.nx != f[0]->p.nx || f[1]->p.ny != f[0]->p.ny || f[1]->p.device != f[0]->p.device ||
        (f[1]->p.flags & LB_FLAG_PLANAR) != (f[0]->p.flags & LB_FLAG_PLANAR))
        return fail(LB_ERR_ARG, "%s: the two lattices of a colony must share grid (geometry), layout flag and device", what);
    return LB_OK;
}

// (src = the current lattice, dst = the other one: what the fused steps read and write; the stages set dst themselves.  Every derived
//  scalar is one float32 operation, here and nowhere else: rocket_launch.h)
static RyArgs rocket_args(lb_sim **f)
{
    RyArgs m = {};
    for (int i = 0; i < 2; ++i) m.a[i] = step_args(f[i], 0, 1, f[i]->H);
    const lb_rocket_params &r = f[0]->ry;
    const float cs = (float)(1.0 / sqrt(3.0));          // np.float32(1. / np.sqrt(3))
    const float cs2 = cs * cs;
    m.inv_cs2 = (float)(1.0 / (double)cs2);             // the kernels' `1. / (cs * cs)`: a double quotient rounded once
    m.G = r.G; m.Gc = r.G_c;
    m.ke = (-r.epsilon) * m.inv_cs2;
    m.ngc = -r.G_chen;
    m.rho_o = r.rho_o; m.c_o = r.c_o; m.alpha = r.alpha;
    m.op = f[0]->ry_op;
    m.Fx = f[0]->pm_G[0]; m.Fy = f[0]->pm_G[1];
    m.Sx = f[0]->pm_ub[0]; m.Sy = f[0]->pm_ub[1];
    return m;
}

static bool ry_finite(float x) { return fabsf(x) <= 3.0e38f; }      // (false for NaN)

int lb_set_rocket(lb_sim **fields, int count, const lb_rocket_params *params)
{
    int rc = rocket_members(fields, count, "lb_set_rocket");
    if (rc) return rc;
    if (!params) return fail(LB_ERR_ARG, "lb_set_rocket: null parameters");
    const lb_rocket_params &r = *params;
    if (r.mode != LB_ROCKET_FLOW && r.mode != LB_ROCKET_FORCES) return fail(LB_ERR_ARG, "lb_set_rocket: unknown mode %d (LB_ROCKET_FLOW and LB_ROCKET_FORCES are built)", r.mode);
    for (float x : {r.G, r.G_c, r.epsilon, r.rho_o, r.G_chen, r.c_o, r.alpha})
        if (!ry_finite(x)) return fail(LB_ERR_ARG, "lb_set_rocket: the parameters must be finite");
    if (r.mode == LB_ROCKET_FLOW && r.rho_o == 0.f) return fail(LB_ERR_ARG, "lb_set_rocket: LB_ROCKET_FLOW needs rho_o != 0");
    if (r.mode == LB_ROCKET_FORCES && r.c_o == 0.f) return fail(LB_ERR_ARG, "lb_set_rocket: LB_ROCKET_FORCES needs c_o != 0");
    fields[0]->ry = r;
    return LB_OK;
}

int lb_get_rocket(lb_sim *first, lb_rocket_params *params)
{
    if (!first || !params) return fail(LB_ERR_ARG, "null argument");
    if (first->cpu || !first->rocket()) return fail(LB_ERR_STATE, "lb_get_rocket is for the lattices of a surfactant-propelled colony (LB_SEM_ROCKET)");
    *params = first->ry;
    return LB_OK;
}

int lb_run_rocket(lb_sim **fields, int count, int n_steps)
{
    int rc = rocket_members(fields, count, "lb_run_rocket");
    if (rc) return rc;
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (n_steps == 0) return LB_OK;
    lb_sim *s0 = fields[0];
    DeviceGuard guard(s0->p.device);
    if ((rc = coupled_join(fields, 2))) return rc;
    const int mode = s0->ry.mode;
    for (int it = 0; it < n_steps; ++it) {
        const RyArgs m = rocket_args(fields);
        const bool last = it == n_steps - 1;            // the last launch stores rho, u, v, psi / S and the forces
        if (rocket_one_launch(s0)) {                    // (the set's first handle chooses: lb_set_variant; plan.cpp)
            lbk_ry_step(mode, last, s0->stream, m);
            HIP_TRY(hipGetLastError());
        } else {
            lbk_ry_moments(s0->stream, m);
            HIP_TRY(hipGetLastError());
            lbk_ry_collide(mode, last, s0->stream, m);
            HIP_TRY(hipGetLastError());
        }
        for (int i = 0; i < 2; ++i) fields[i]->cur ^= 1;
    }
    for (int i = 0; i < 2; ++i) {
        fields[i]->feq_valid = false;
        fields[i]->macro_valid = true;
    }
    return coupled_release(fields, 2);
}

int lb_update_velocity_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_update_velocity_rocket");
    if (rc) return rc;
    DeviceGuard guard(fields[0]->p.device);
    if ((rc = coupled_join(fields, 2))) return rc;
    lbk_ry_velocity(fields[0]->ry.mode, fields[0]->stream, rocket_args(fields));
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < 2; ++i) fields[i]->feq_valid = false;
    return coupled_release(fields, 2);
}

int lb_update_forces_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_update_forces_rocket");
    if (rc) return rc;
    DeviceGuard guard(fields[0]->p.device);
    if ((rc = coupled_join(fields, 2))) return rc;
    lbk_ry_forces(fields[0]->ry.mode, fields[0]->stream, rocket_args(fields));
    HIP_TRY(hipGetLastError());
    return coupled_release(fields, 2);
}

int lb_collide_rocket(lb_sim **fields, int count)
{
    int rc = rocket_members(fields, count, "lb_collide_rocket");
    if (rc) return rc;
    for (int i = 0; i < 2; ++i)
        if (!fields[i]->feq) return fail(LB_ERR_STATE, "lb_collide_rocket before lb_update_feq on both members");
    DeviceGuard guard(fields[0]->p.device);
    if ((rc = coupled_join(fields, 2))) return rc;
    RyArgs m = rocket_args(fields);
    for (int i = 0; i < 2; ++i) m.a[i].dst = fields[i]->origin(fields[i]->cur);      // relaxed in place
    lbk_ry_relax(fields[0]->ry.mode, fields[0]->stream, m, fields[0]->feq_origin(), fields[1]->feq_origin());
    HIP_TRY(hipGetLastError());
    return coupled_release(fields, 2);
}

int lb_get_rocket_fields(lb_sim **fields, int count, float *psi_or_S, float *Fx, float *Fy, float *Fsx, float *Fsy)
{
    int rc = rocket_members(fields, count, "lb_get_rocket_fields");
    if (rc) return rc;
    lb_sim *s = fields[0];
    DeviceGuard guard(s->p.device);
    float *out[5] = {psi_or_S, Fx, Fy, Fsx, Fsy};
    const float *from[5] = {s->ry_op, s->pm_G[0], s->pm_G[1], s->pm_ub[0], s->pm_ub[1]};
    for (int i = 0; i < 5; ++i)
        if (out[i] && (rc = copy_plane_d2h(s, out[i], from[i]))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

// ---- health check ------------------------------------------------------------------------
int lb_check(lb_sim *s, int across_ranks, int64_t *n_nonfinite, float *max_mach, double *sum_rho)
{
    if (s && s->cpu) {
        if (across_ranks) return fail(LB_ERR_STATE, "lb_check across ranks is not available on the CPU backend");
        const size_t n = s->cpu->plane();
        const float *f = s->cpu->f.data();
        int64_t bad = 0;
        double sum = 0.;
        float mx = 0.f;
        for (size_t c = 0; c < n; ++c) {                // the moments of the populations, as the device pass computes them
            float r = f[c];
            for (int k = 1; k < 9; ++k) r += f[k * n + c];
            const float inv = 1.f / r;
            const float ux = (f[n + c] - f[3 * n + c] + f[5 * n + c] - f[6 * n + c] - f[7 * n + c] + f[8 * n + c]) * inv;
            const float uy = (f[5 * n + c] + f[2 * n + c] + f[6 * n + c] - f[7 * n + c] - f[4 * n + c] - f[8 * n + c]) * inv;
            const float usq = ux * ux + uy * uy;
            if (fabsf(r) <= 3.0e38f && fabsf(usq) <= 3.0e38f) { sum += (double)r; mx = fmaxf(mx, usq); }
            else ++bad;
        }
        if (n_nonfinite) *n_nonfinite = bad;
        if (max_mach) *max_mach = sqrtf(3.f * mx);
        if (sum_rho) *sum_rho = sum;
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_check inside a split step");
    if (s->poisson()) return fail(LB_ERR_STATE, "lb_check is not available on the LB Poisson solver (LB_SEM_POISSON): lb_solve reports its residual");
    NOT_POROUS(s, "lb_check");
    if (across_ranks && !s->comm) return fail(LB_ERR_STATE, "lb_check across ranks needs lb_comm_init");
    DeviceGuard guard(s->p.device);
    // the pass that rebuilds rho, u, v reduces the same three numbers: one pass serves both when the fields are due (never on a
    // scalar lattice, whose rho is stored by its runs and whose u, v are imposed: macro_valid stays true there)
    int rc = check_pass(s, !s->macro_valid && lazy_macro(s));
    if (rc) return rc;
    s->macro_valid = true;
    CheckPartial *res = s->check_part + (s->check_cap - 1);
    CheckPartial h;
    if (across_ranks) {
        // sum_rho and the count travel as two doubles (exact up to 2^53 cells), the maximum on its own
        double *d = reinterpret_cast<double *>(s->halo_buf);             // (>= 4 x 81 x nx floats, free between runs)
        float *m = reinterpret_cast<float *>(d + 4);
        hipLaunchKernelGGL(k_check_spread, dim3(1), dim3(1), 0, s->stream, (const CheckPartial *)res, d, m);
        HIP_TRY(hipGetLastError());
        NCCL_TRY(g_rccl.AllReduce(d, d + 2, 2, ncclFloat64, ncclSum, s->comm, s->stream));
        NCCL_TRY(g_rccl.AllReduce(m, m + 1, 1, ncclFloat32, ncclMax, s->comm, s->stream));
        double hd[2];
        float hm;
        HIP_TRY(hipMemcpyAsync(hd, d + 2, sizeof(hd), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(&hm, m + 1, sizeof(hm), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        h.sum_rho = hd[0]; h.nonfinite = (unsigned long long)hd[1]; h.max_usq = hm;
    } else {
        HIP_TRY(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (n_nonfinite) *n_nonfinite = (int64_t)h.nonfinite;
    if (max_mach) *max_mach = sqrtf(3.f * h.max_usq);                   // |u| / c_s, c_s = 1 / sqrt(3)
    if (sum_rho) *sum_rho = h.sum_rho;
    return LB_OK;
}

// ---- measurement: the planner's answers (plan.cpp) ------------------------------------------
int lb_plan_launches(lb_sim *s, int n_steps, int *depths, int max_launches)
{
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (s->cpu || s->p.semantics == LB_SEM_CYTHON || s->multi_slab()) return LB_ERR_STATE;     // (whole-grid OpenCL-path GPU handles)
    return plan_launches(s, n_steps, depths, max_launches);
}

int lb_steps_per_launch(lb_sim *s)
{
    if (s && s->cpu) return 1;
    if (!s) return fail(LB_ERR_ARG, "null handle");
    return steps_per_launch(s);
}

int lb_hot_kernel(lb_sim *s, char *buf, int buflen)
{
    if (s && s->cpu) {
        if (!buf || buflen < 1) return fail(LB_ERR_ARG, "bad argument");
        snprintf(buf, (size_t)buflen, "cpu backend (cython_dim.pyx Pipe_Flow.run restated for the host, 1 thread)");
        return LB_OK;
    }
    if (!s || !buf || buflen < 1) return fail(LB_ERR_ARG, "bad argument");
    hot_kernel(s, buf, buflen);
    return LB_OK;
}

int lb_copy_calibration(lb_sim *s, int nontemporal, int64_t *bytes_moved)
{
    CPU_UNSUPPORTED(s, "lb_copy_calibration");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_copy_calibration inside a split step");
    DeviceGuard guard(s->p.device);
    const long long n4 = s->lat_floats / 4;
    const f4a *src = reinterpret_cast<const f4a *>(s->lat[s->cur]);
    f4a *dst = reinterpret_cast<f4a *>(s->lat[s->cur ^ 1]);
    const unsigned grid = (unsigned)((n4 + 255) / 256);   // one float4 per thread
    if (nontemporal) hipLaunchKernelGGL(k_copy4<true>, dim3(grid), dim3(256), 0, s->stream, src, dst, n4);
    else hipLaunchKernelGGL(k_copy4<false>, dim3(grid), dim3(256), 0, s->stream, src, dst, n4);
    HIP_TRY(hipGetLastError());
    if (bytes_moved) *bytes_moved = 2 * n4 * 16;
    return LB_OK;
}

int lb_timer_start(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->t0 = std::chrono::steady_clock::now(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipEventRecord(s->ev_t0, s->stream));
    return LB_OK;
}

int lb_timer_stop(lb_sim *s, float *elapsed_ms)
{
    if (s && s->cpu) {
        if (!elapsed_ms) return fail(LB_ERR_ARG, "null argument");
        *elapsed_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - s->cpu->t0).count();
        return LB_OK;
    }
    if (!s || !elapsed_ms) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipEventRecord(s->ev_t1, s->stream));
    HIP_TRY(hipEventSynchronize(s->ev_t1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, s->ev_t0, s->ev_t1));
    return LB_OK;
}

}  // extern "C"

