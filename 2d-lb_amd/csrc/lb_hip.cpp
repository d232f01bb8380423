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
// plain C++), launch.cpp (the flow launches), slab.cpp (halo exchange and the slab schedules), transport.cpp (RCCL, peer set-up),
// tune.cpp (lb_autotune*), one unit per handle kind other than flow (scalar.cpp ... rocket.cpp: its kernels, its row of the kind table,
// its own entry points), and this file: the handle's life, state transfer, the entry points every kind shares -- common checks, then the
// kind's row --, the flow kind's row with its un-fused phases and the Cython path (kernels_phases.h), the health check (kernels_check.h),
// lb_run_batch and what set calls share, timers.
// All stores of the fused kernel are 16-byte aligned; the six planes with cx != 0 are read through
// 16-byte loads that are misaligned by one element (gfx950 global loads only need dword alignment).
#include "host.h"

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

}  // namespace

bool finite32(float x) { return fabsf(x) <= 3.0e38f; }

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
int copy_quads(hipStream_t st, float *dst, const float *src, long long n4)
{
    hipLaunchKernelGGL(k_copy4<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const f4a *>(src), reinterpret_cast<f4a *>(dst), n4);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}
static int copy_lattice(lb_sim *s, float *dst, const float *src) { return copy_quads(s->stream, dst, src, s->lat_floats / 4); }    // (lat_floats is a multiple of 64)

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
static int lattice_plane_h2d(lb_sim *s, float *origin, int k, const float *host)
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
static int lattice_plane_d2h(lb_sim *s, float *host, const float *origin, int k)
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
static int frozen_links(lb_sim *s, int which, bool patch)
{
    if (s->p.bc_mode == LB_BC_VELOCITY_INLET || s->p.bc_mode == LB_BC_BOX || s->p.bc_mode == LB_BC_DIRICHLET) {
        const int X = s->p.nx - 1, Y = s->p.ny - 1;
        struct Link { int k, x, y; };
        const Link vel[8] = {{1, 0, 0}, {8, 0, 0}, {1, 0, Y}, {5, 0, Y}, {3, X, 0}, {7, X, 0}, {3, X, Y}, {6, X, Y}};   // (bc_vel_cell's order)
        const Link box[8] = {{6, 0, 0}, {8, 0, 0}, {5, X, 0}, {7, X, 0}, {5, 0, Y}, {7, 0, Y}, {6, X, Y}, {8, X, Y}};   // (MfBox's and PsBox's order)
        const Link *c = s->p.bc_mode == LB_BC_VELOCITY_INLET ? vel : box;
        for (int i = 0; i < 8; ++i) {
            float *in_lat = s->origin(which) + c[i].k * s->plane + (long long)c[i].y * s->rowp + c[i].x, *kept = s->vi_corner + i;
            HIP_TRY(hipMemcpyAsync(patch ? in_lat : kept, patch ? kept : in_lat, sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        }
    } else if (s->ad_edge) {
        const StepArgs a = step_args(s, 0, 1, s->H);
        lbk_ad_edge(patch, s->stream, a, s->origin(which), s->ad_edge);
        HIP_TRY(hipGetLastError());
    }
    return LB_OK;
}
// ... whenever the populations are set as a whole (lb_set_f, lb_init_pop)
static int frozen_capture(lb_sim *s, int which) { return frozen_links(s, which, false); }
// ... behind the un-fused streaming phase (lb_move), where the boundary phase reads them
static int frozen_patch(lb_sim *s, int which) { return frozen_links(s, which, true); }

// lb_run in Cython-path semantics
static int run_cython(lb_sim *s, int n_steps)
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

// ---- the flow kind's row: the un-fused phases of the three flow semantics, lb_run's dispatch -------------------------------------------
static int flow_move_bcs(lb_sim *s)
{
    int rc = ensure_macro(s);
    if (rc) return rc;
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

static int flow_hydro(lb_sim *s)
{
    if (s->p.semantics == LB_SEM_CYTHON)
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
    return LB_OK;
}

static int flow_feq(lb_sim *s)
{
    PhaseArgs a = phase_args(s);
    a.ny = s->H;   // rho,u,v are local: valid for slabs too
    if (s->p.semantics == LB_SEM_OPENCL_D2Q9I)
        hipLaunchKernelGGL(k_feq_i, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    else
        hipLaunchKernelGGL(k_feq, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int collide_ready(lb_sim *s)
{
    if (!s->feq) return fail(LB_ERR_STATE, "lb_collide_particles before any lb_update_feq");
    return ensure_macro(s);
}

static int flow_collide(lb_sim *s)
{
    if (int rc = collide_ready(s)) return rc;
    hipLaunchKernelGGL(k_collide, cells_grid(s, 9), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

static int run_flow(lb_sim *s, int n_steps)
{
    if (!s->tune_cache_checked) (void)tune_cache_apply(s);
    if (s->p.semantics == LB_SEM_CYTHON) return run_cython(s, n_steps);
    if (!s->multi_slab()) return run_whole_grid(s, n_steps);     // (never blocks the host: tuning is lb_autotune*'s job)
    return run_slab(s, n_steps);
}

KIND_ROW(kind_flow, nullptr, 0, nullptr, false, false, 0, nullptr, 0, nullptr, flow_move_bcs, flow_hydro, flow_feq, flow_collide, run_flow)

const KindOps &kind_of(int semantics)
{
    switch (semantics) {
    case LB_SEM_DIFFUSION: return kind_scalar();
    case LB_SEM_MULTIFIELD: return kind_multifield();
    case LB_SEM_POISSON: return kind_poisson();
    case LB_SEM_POROUS: return kind_porous();
    case LB_SEM_MULTIFLUID: return kind_multifluid();
    case LB_SEM_ROCKET: return kind_rocket();
    default: return kind_flow();
    }
}

// What lb_create refuses of a kind other than flow (KindOps, host.h), before any device is touched.
static int kind_refusals(const KindOps &k, const lb_params *p)
{
    if (!(k.families >> p->bc_mode & 1u)) {
        if (&k == &kind_poisson()) return fail(LB_ERR_ARG, "%s takes %s: unknown semantics %d for bc_mode %d", k.noun, k.families_text, p->semantics, p->bc_mode);
        return fail(LB_ERR_ARG, "%s takes %s", k.noun, k.families_text);
    }
    if (&k == &kind_porous() && p->bc_mode == LB_BC_ZERO_GRADIENT && (p->nx < 3 || p->ny < 3))
        return fail(LB_ERR_ARG, "LB_BC_ZERO_GRADIENT needs an interior cell: grid must be at least 3x3 (got %dx%d)", p->nx, p->ny);
    if (k.eight_neighbours && (p->nx < 3 || p->ny < 3))
        return fail(LB_ERR_ARG, "%s needs a cell with eight neighbours: grid must be at least 3x3 (got %dx%d)", k.noun, p->nx, p->ny);
    if (p->local_ny != p->ny || p->y0 != 0) return fail(LB_ERR_ARG, "%s owns its whole grid: no slabs", k.noun);
    if (p->flags & LB_FLAG_HALO) return fail(LB_ERR_ARG, "%s has no halo interface (LB_FLAG_HALO)", k.noun);
    if (p->device == LB_DEVICE_CPU) return fail(LB_ERR_ARG, "%s runs on a GPU only (no CPU backend)", k.noun);
    return LB_OK;
}

// ---- what set calls share (host.h) ---------------------------------------------------------------------------------------------------
SetFault set_fault(lb_sim **f, int count, int semantics, bool rocket_named, bool split_checked, int *at)
{
    for (int i = 0; i < count; ++i) {
        const lb_sim *s = f[i];
        *at = i;
        if (!s) return SET_NULL_MEMBER;
        if (rocket_named && s->rocket()) return SET_ROCKET_NAMED;
        if (s->cpu || s->p.semantics != semantics) return SET_KIND;
        if (!same_geometry(s, f[0])) return SET_GEOMETRY;
        if (split_checked && s->stepping) return SET_SPLIT_STEP;
        for (int j = 0; j < i; ++j)
            if (f[j] == s) return SET_TWICE;
    }
    return SET_FINE;
}

int SetScope::join()
{
    for (int i = 1; i < count; ++i) {
        HIP_TRY(hipEventRecord(f[i]->ev_interior, f[i]->stream));
        HIP_TRY(hipStreamWaitEvent(f[0]->stream, f[i]->ev_interior, 0));
    }
    joined = true;
    return LB_OK;
}

int SetScope::release()
{
    joined = false;
    if (count < 2) return LB_OK;
    HIP_TRY(hipEventRecord(f[0]->ev_interior, f[0]->stream));
    for (int i = 1; i < count; ++i) HIP_TRY(hipStreamWaitEvent(f[i]->stream, f[0]->ev_interior, 0));
    return LB_OK;
}

SetScope::~SetScope()
{
    if (!joined || count < 2) return;
    (void)hipEventRecord(f[0]->ev_interior, f[0]->stream);
    for (int i = 1; i < count; ++i) (void)hipStreamWaitEvent(f[i]->stream, f[0]->ev_interior, 0);
}

// The buffers every GPU handle has, the kind's own among them (KindOps::create).  A failure leaves what was allocated to lb_destroy.
static int create_device(lb_sim *s)
{
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
    const KindOps &k = kind_of(s);
    if (k.create && k.create(s)) return LB_ERR_HIP;
    CREATE_TRY(hipMalloc(&s->vi_corner, 8 * sizeof(float)));
    CREATE_TRY(hipMemsetAsync(s->vi_corner, 0, 8 * sizeof(float), s->stream));
    CREATE_TRY(hipMalloc(&s->mask_raw, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD));
    s->mask = s->mask_raw + GUARD + MASK_GHOST * s->pitch;
    CREATE_TRY(hipMemsetAsync(s->rho, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->u, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->v, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->mask_raw, 0, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD, s->stream));
    CREATE_TRY(hipStreamSynchronize(s->stream));
    s->bytes += 2 * lat_bytes + 3 * fld_bytes + (size_t)s->pitch * s->H;
    return LB_OK;
}

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
    // a kind other than flow: a whole-grid GPU handle without obstacles, refused from its row before any device is touched
    const KindOps &k = kind_of(p->semantics);
    int rc;
    if (k.noun && k.before_exists && (rc = kind_refusals(k, p))) return rc;
    if (p->bc_mode == LB_BC_OPEN && p->semantics != LB_SEM_DIFFUSION)
        return fail(LB_ERR_ARG, "LB_BC_OPEN exists for scalar lattices (LB_SEM_DIFFUSION) only");
    if (p->bc_mode == LB_BC_BOX && p->semantics != LB_SEM_MULTIFIELD)
        return fail(LB_ERR_ARG, "bc_mode LB_BC_BOX exists for coupled scalar lattices (LB_SEM_MULTIFIELD) only");
    if (k.noun && !k.before_exists && (rc = kind_refusals(k, p))) return rc;
    if (p->bc_mode == LB_BC_VELOCITY_INLET &&
        (p->local_ny != p->ny || (p->flags & LB_FLAG_HALO) || p->semantics != LB_SEM_OPENCL))
        return fail(LB_ERR_ARG, "the velocity-inlet family exists for whole-grid OpenCL-path handles only");
    if (p->bc_mode == LB_BC_VELOCITY_INLET && (!(p->inlet_u < 1.f) || !(p->outlet_u > -1.f)))
        return fail(LB_ERR_ARG, "velocity-inlet speeds must satisfy inlet_u < 1 and outlet_u > -1");
    if (!(p->omega > 0.f && p->omega < 2.f)) return fail(LB_ERR_ARG, "omega must be in (0,2), got %g", p->omega);
    for (int r : p->reserved)
        if (r != 0) return fail(LB_ERR_ARG, "reserved fields must be zero");
    if (p->flags & ~(LB_FLAG_HALO | LB_FLAG_PLANAR | LB_FLAG_EAGER_MACRO)) return fail(LB_ERR_ARG, "unknown flags 0x%x", p->flags);
    if (!k.noun && p->semantics != LB_SEM_OPENCL && p->semantics != LB_SEM_CYTHON && p->semantics != LB_SEM_OPENCL_D2Q9I)
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

    if (create_device(s)) {
        lb_destroy(s);
        return LB_ERR_HIP;
    }
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
    for (float *p : {s->lat[0], s->lat[1], s->feq, s->rho, s->u, s->v, s->halo_buf, s->vi_corner, s->stage, s->ad_edge, s->ad_noise_field, s->ps_source, s->ps_part,
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
    const KindOps &k = kind_of(s);
    if (k.variant_text && (variant < -1 || variant > k.variant_max)) return fail(k.variant_code, "%s", k.variant_text);
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
    const KindOps &k = kind_of(s);
    if (!k.move_bcs) return LB_OK;
    DeviceGuard guard(s->p.device);
    return k.move_bcs(s);
}

int lb_update_hydro(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->update_hydro(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_update_hydro");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    if ((rc = kind_of(s).hydro(s))) return rc;
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
    if ((rc = kind_of(s).feq(s))) return rc;
    s->feq_valid = true;
    return LB_OK;
}

int lb_collide_particles(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->collide(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_collide_particles");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    return kind_of(s).collide(s);
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
    DeviceGuard guard(s->p.device);
    return kind_of(s).run(s, n_steps);
}

// Population sets: `count` periodic whole-grid lattices of one geometry (one per population of a multi-population
// model, each with its own omega / mask content) advanced in lock step, ONE launch per time step for all of them.
int lb_run_batch(lb_sim **sims, int count, int n_steps)
{
    for (int i = 0; sims && i < count; ++i) CPU_UNSUPPORTED(sims[i], "lb_run_batch");
    for (int i = 0; sims && i < count; ++i) SCALAR_UNSUPPORTED(sims[i], "lb_run_batch");
    if (!sims || count < 1 || count > BATCH_MAX || n_steps < 0)
        return fail(LB_ERR_ARG, "lb_run_batch takes 1..%d handles and a non-negative step count", BATCH_MAX);
    // (not set_fault's rules: the kind is a whole-grid periodic flow handle, and what the members share is grid, device and mask presence)
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
    SetScope sc(sims, count);
    if (int rc = sc.join()) return rc;
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
    for (int i = 0; i < count; ++i) {
        sims[i]->feq_valid = false;
        sims[i]->macro_valid = !lazy;
    }
    return sc.release();
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
            if (finite32(r) && finite32(usq)) { sum += (double)r; mx = fmaxf(mx, usq); }
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

