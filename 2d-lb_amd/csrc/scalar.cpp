// scalar.cpp -- scalar lattices (LB_SEM_DIFFUSION): the kernels of kernels_scalar.h and their launches, the kind's row of the kind table
// (host.h: KindOps), its run, and the entry points of the C ABI that are its own: lb_set_reaction, the edge state, lb_set_velocity_from,
// the noisy collision (lb_set_noise ...: the stream is philox.h's, the noise counter ad_t advances by one per noisy collision).
#include "kernels_scalar.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

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

// the noisy instantiations (always with the growth term: G = 0 adds nothing)
template <int BC, bool RHO, typename NZ>
void ad_noisy_tile_go(int shape, hipStream_t st, const StepArgs &a, const AdExtra &e, const NZ &nz)
{
    with_tile_shape(shape, a.nx, a.ny, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_ad_tile4<BC, true, RHO, T::TW, T::TH, T::CPT, NZ>), t.grid, t.block, 0, st, a, e, t.tiles_x, t.n_tiles, nz);
    });
}

template <typename NZ>
void ad_noisy_tile_plan(int bc, bool store_rho, int shape, hipStream_t st, const StepArgs &a, const AdExtra &e, const NZ &nz)
{
    if (bc == LB_BC_PERIODIC) {
        if (store_rho) ad_noisy_tile_go<LB_BC_PERIODIC, true>(shape, st, a, e, nz);
        else ad_noisy_tile_go<LB_BC_PERIODIC, false>(shape, st, a, e, nz);
    } else {
        if (store_rho) ad_noisy_tile_go<LB_BC_OPEN, true>(shape, st, a, e, nz);
        else ad_noisy_tile_go<LB_BC_OPEN, false>(shape, st, a, e, nz);
    }
}

// per_cell: the per-cell plan (an explicit variant with LB_VAR_STEP4_NO_AHEAD: the A/B switch) instead of the noise plane in LDS
void ad_noisy_tile4(int bc, bool store_rho, int shape, bool per_cell, hipStream_t st, const StepArgs &a, const AdExtra &e, const AdNoise &nz)
{
    if (per_cell) {
        AdNoiseCell c;
        static_cast<AdNoise &>(c) = nz;
        ad_noisy_tile_plan(bc, store_rho, shape, st, a, e, c);
    } else {
        ad_noisy_tile_plan(bc, store_rho, shape, st, a, e, nz);
    }
}

void ad_noisy_step(int bc, bool store_rho, hipStream_t st, const StepArgs &a, const AdExtra &e, const AdNoise &nz)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (bc == LB_BC_PERIODIC) {
        if (store_rho) hipLaunchKernelGGL((k_ad_step<LB_BC_PERIODIC, true, true, AdNoise>), grid, block, 0, st, a, e, nz);
        else hipLaunchKernelGGL((k_ad_step<LB_BC_PERIODIC, true, false, AdNoise>), grid, block, 0, st, a, e, nz);
    } else {
        if (store_rho) hipLaunchKernelGGL((k_ad_step<LB_BC_OPEN, true, true, AdNoise>), grid, block, 0, st, a, e, nz);
        else hipLaunchKernelGGL((k_ad_step<LB_BC_OPEN, true, false, AdNoise>), grid, block, 0, st, a, e, nz);
    }
}

// the handle's noise as a launch takes it: the stream at the handle's counter
AdNoise ad_noise_of(const lb_sim *s) { return AdNoise{s->ad_Dg, s->ad_seed, s->ad_t, nullptr}; }
const char *const NOISE_FIELD_SET = "a noise field is set (lb_set_noise_field): only lb_collide_particles uses one; drop it with NULL first";

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

// bc: LB_BC_PERIODIC or LB_BC_OPEN.  k_ad_tile4: four steps over the whole grid; shape 0: 32 x 16 tiles, two cells per thread; 1: 32 x 16,
// one; 2: 16 x 16, one.  store_rho: the launch also stores rho.
void ad_tile4(int bc, bool react, bool store_rho, int shape, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    if (bc == LB_BC_PERIODIC) ad_tile_bc<LB_BC_PERIODIC>(react, store_rho, shape, st, a, e);
    else ad_tile_bc<LB_BC_OPEN>(react, store_rho, shape, st, a, e);
}

// k_ad_step over the whole grid
void ad_step(int bc, bool react, bool store_rho, hipStream_t st, const StepArgs &a, const AdExtra &e)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (bc == LB_BC_PERIODIC) ad_step_go<LB_BC_PERIODIC>(react, store_rho, grid, block, st, a, e);
    else ad_step_go<LB_BC_OPEN>(react, store_rho, grid, block, st, a, e);
}

int scalar_create(lb_sim *s)
{
    if (s->p.bc_mode != LB_BC_OPEN) return LB_OK;
    const size_t edge_bytes = sizeof(float) * (size_t)ad_edge_device_floats(s->pitch, s->p.ny);
    CREATE_TRY(hipMalloc(&s->ad_edge, edge_bytes));
    CREATE_TRY(hipMemsetAsync(s->ad_edge, 0, edge_bytes, s->stream));
    return LB_OK;
}

// f (in place) relaxed towards feq
int scalar_collide(lb_sim *s)
{
    int rc = collide_ready(s);
    if (rc) return rc;
    if (s->ad_Dg != 0.f && s->p.semantics == LB_SEM_DIFFUSION) {       // the stream, or the supplied field in its place; either way one noisy collision
        AdNoise nz = ad_noise_of(s);
        nz.field = s->ad_noise_field;
        if ((rc = launch_phase(s, grid_cells(s), k_ad_collide<true, AdNoise>, s->origin(s->cur), s->feq_origin(), s->ad_G, nz))) return rc;
        s->ad_t += 1;
        return LB_OK;
    }
    return launch_phase(s, grid_cells(s), s->ad_G != 0.f ? k_ad_collide<true> : k_ad_collide<false>, s->origin(s->cur), s->feq_origin(), s->ad_G);
}

// n time steps: k_ad_tile4 / k_ad_step launch by launch, as scalar_next_advance splits the run; the last launch stores rho (with a
// growth term rho is not a moment of the populations a run leaves behind: never rebuilt on demand)
int run_scalar(lb_sim *s, int n_steps)
{
    const AdExtra e = AdExtra{s->ad_edge, s->ad_G};
    const bool noisy = s->ad_Dg != 0.f;
    if (noisy && s->ad_noise_field) return fail(LB_ERR_STATE, "lb_run: %s", NOISE_FIELD_SET);
    int left = n_steps;
    while (left > 0) {
        const int adv = scalar_next_advance(s, left);
        const StepArgs a = step_args(s, 0, 1, s->H);
        if (noisy) {            // step i of a launch draws at counter t + i
            if (adv == TILE_T) ad_noisy_tile4(s->p.bc_mode, left == adv, scalar_tile_shape(s), s->variant >= 0 && (s->variant & LB_VAR_STEP4_NO_AHEAD), s->stream, a, e, ad_noise_of(s));
            else ad_noisy_step(s->p.bc_mode, left == adv, s->stream, a, e, ad_noise_of(s));
        } else if (adv == TILE_T) ad_tile4(s->p.bc_mode, s->ad_G != 0.f, left == adv, scalar_tile_shape(s), s->stream, a, e);
        else ad_step(s->p.bc_mode, s->ad_G != 0.f, left == adv, s->stream, a, e);
        HIP_TRY(hipGetLastError());
        s->cur ^= 1;
        if (noisy) s->ad_t += (unsigned long long)adv;
        left -= adv;
    }
    if (n_steps) { s->feq_valid = false; s->macro_valid = true; }
    return LB_OK;
}

}  // namespace

int scalar_hydro(lb_sim *s) { return launch_phase(s, grid_cells(s), k_ad_hydro); }       // rho only: u, v are imposed
int scalar_feq(lb_sim *s) { return launch_phase(s, grid_cells(s), k_ad_feq, s->feq_origin()); }

int scalar_moments(lb_sim *s)
{
    const StepArgs a = step_args(s, 0, 1, s->H);
    const AdExtra e = AdExtra{s->ad_edge, s->ad_G};
    if (s->p.bc_mode == LB_BC_PERIODIC) hipLaunchKernelGGL(k_ad_moments<LB_BC_PERIODIC>, step_grid(a), dim3(64, 4), 0, s->stream, a, e);
    else hipLaunchKernelGGL(k_ad_moments<LB_BC_OPEN>, step_grid(a), dim3(64, 4), 0, s->stream, a, e);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int scalar_step(lb_sim *s, bool store_rho)
{
    if (s->ad_Dg != 0.f) {
        if (s->ad_noise_field) return fail(LB_ERR_STATE, "%s", NOISE_FIELD_SET);
        ad_noisy_step(s->p.bc_mode, store_rho, s->stream, step_args(s, 0, 1, s->H), AdExtra{s->ad_edge, s->ad_G}, ad_noise_of(s));
        s->ad_t += 1;
    } else {
        ad_step(s->p.bc_mode, s->ad_G != 0.f, store_rho, s->stream, step_args(s, 0, 1, s->H), AdExtra{s->ad_edge, s->ad_G});
    }
    HIP_TRY(hipGetLastError());
    s->cur ^= 1;
    return LB_OK;
}

int scalar_step_carried(lb_sim *s, const lb_sim *flow, bool store_rho)
{
    StepArgs a = step_args(s, 0, 1, s->H);
    a.u = flow->u;              // (same pitch: same nx)
    a.v = flow->v;
    ad_step(LB_BC_PERIODIC, s->ad_G != 0.f, store_rho, flow->stream, a, AdExtra{s->ad_edge, s->ad_G});
    HIP_TRY(hipGetLastError());
    s->cur ^= 1;
    return LB_OK;
}

void lbk_ad_edge(bool patch,hipStream_t st, const StepArgs &a, float *f, float *edge)
{
    const int n = std::max(patch ? a.nx : a.fpitch, a.ny);      // (the capture takes the rows' padding along)
    if (patch) hipLaunchKernelGGL(k_ad_edge_patch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, f, (const float *)edge);
    else hipLaunchKernelGGL(k_ad_edge_capture, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, (const float *)f, edge);
}

long long ad_check_blocks(const StepArgs &a) { return (long long)((a.nx + 255) / 256) * a.ny; }

void lbk_ad_check(hipStream_t st, const StepArgs &a, CheckPartial *part)
{
    hipLaunchKernelGGL(k_ad_check, cells_grid(a), dim3(256), 0, st, a, part);
}

// (move_bcs: diffusion.py:326-331, `pass`)
KIND_ROW(kind_scalar,
    "a scalar lattice (LB_SEM_DIFFUSION)", 1u << LB_BC_PERIODIC | 1u << LB_BC_OPEN, "the families LB_BC_PERIODIC and LB_BC_OPEN only", false, false,
    0, nullptr, 0,
    scalar_create, nullptr, scalar_hydro, scalar_feq, scalar_collide, run_scalar)

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

extern "C" {

int lb_set_reaction(lb_sim *s, float G)
{
    NEED_SCALAR(s, "lb_set_reaction");
    NOT_POISSON(s, "lb_set_reaction");
    if (!finite32(G)) return fail(LB_ERR_ARG, "the growth rate must be finite");
    s->ad_G = G;
    return LB_OK;
}

// ABI order of the edge state (include/lb_hip.h: west, east, south, north; unpadded) <-> device order (scalar_launch.h)
int lb_edge_floats(lb_sim *s)
{
    NEED_SCALAR(s, "lb_edge_floats");
    return (int)(s->ad_edge ? 6LL * (s->p.nx + s->p.ny) : 0);
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

// ---- the noisy collision (collide_particles_noisy_fisher): LB_SEM_DIFFUSION handles only ------------------------------------------
#define NEED_DIFFUSION(s, name)                                                                              \
    do {                                                                                                     \
        NEED_SCALAR(s, name);                                                                                \
        if ((s)->p.semantics != LB_SEM_DIFFUSION)                                                            \
            return fail(LB_ERR_STATE, "%s is for scalar lattices on their own (LB_SEM_DIFFUSION)", name);    \
    } while (0)

int lb_set_noise(lb_sim *s, float Dg, uint64_t seed)
{
    NEED_DIFFUSION(s, "lb_set_noise");
    if (!finite32(Dg) || Dg < 0.f) return fail(LB_ERR_ARG, "the noise strength must be finite and not negative");
    s->ad_Dg = Dg;
    s->noisy = Dg != 0.f;       // (the planner's: automatic runs of a noisy handle stay on k_ad_step, plan.cpp)
    s->ad_seed = seed;
    s->ad_t = 0;
    return LB_OK;
}

int lb_get_noise(lb_sim *s, float *Dg, uint64_t *seed, uint64_t *t)
{
    NEED_DIFFUSION(s, "lb_get_noise");
    if (Dg) *Dg = s->ad_Dg;
    if (seed) *seed = s->ad_seed;
    if (t) *t = s->ad_t;
    return LB_OK;
}

int lb_set_noise_counter(lb_sim *s, uint64_t t)
{
    NEED_DIFFUSION(s, "lb_set_noise_counter");
    s->ad_t = t;
    return LB_OK;
}

int lb_noise_fill(lb_sim *s, uint64_t t, float *out, int on_device)
{
    NEED_DIFFUSION(s, "lb_noise_fill");
    if (!out) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    const int nx = s->p.nx, ny = s->p.ny;
    const size_t bytes = sizeof(float) * (size_t)nx * ny;
    float *dev = out;
    if (!on_device) HIP_TRY(hipMalloc(&dev, bytes));
    hipLaunchKernelGGL(k_ad_noise_fill, dim3((unsigned)((nx + 1023) / 1024), (unsigned)ny), dim3(256), 0, s->stream,
                       AdNoise{s->ad_Dg, s->ad_seed, t, nullptr}, nx, dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (!on_device) (void)hipFree(dev);
    if (e != hipSuccess) return fail(LB_ERR_HIP, "lb_noise_fill: %s", hipGetErrorString(e));
    return LB_OK;
}

int lb_set_noise_field(lb_sim *s, const float *z, int on_device)
{
    NEED_DIFFUSION(s, "lb_set_noise_field");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipStreamSynchronize(s->stream));       // (a collision in flight may still be reading the field)
    if (!z) {
        if (s->ad_noise_field) (void)hipFree(s->ad_noise_field);
        s->ad_noise_field = nullptr;
        return LB_OK;
    }
    const size_t bytes = sizeof(float) * (size_t)s->p.nx * s->p.ny;
    if (!s->ad_noise_field) HIP_TRY(hipMalloc(&s->ad_noise_field, bytes));
    HIP_TRY(hipMemcpy(s->ad_noise_field, z, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
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
    // a set of two, the flow handle first: on ITS stream, behind its work; this handle's kernels may still read u, v, and its later ones
    // must see the new
    lb_sim *pair[2] = {flow, s};
    SetScope sc(pair, 2);
    int rc = ensure_macro(flow);                    // the flow's lazily rebuilt rho, u, v
    if (rc) return rc;
    if ((rc = sc.join())) return rc;
    // (rho, u, v are [H][pitch] whatever the layout of the lattices: LB_FLAG_PLANAR on either handle does not matter here)
    const long long n4 = s->pitch * s->H / 4;       // (same pitch: same nx)
    for (int i = 0; i < 2; ++i)
        if ((rc = copy_quads(flow->stream, i ? s->v : s->u, i ? flow->v : flow->u, n4))) return rc;
    s->feq_valid = false;
    return sc.release();
}

}  // extern "C"
