// spectral.cpp -- the spectral screened-Poisson solver (lb_spectral_*: the reference's spectral_poisson/screened_poisson.py) and its
// coupling to a scalar lattice (lb_spectral_velocity, lb_run_screened: reaction_diffusion/screened_poisson_waves.py): the kernels of
// kernels_spectral.h, their launches, the entry points of the C ABI.  An lb_spectral is not a handle kind: it owns three dense complex
// arrays and two twiddle tables, nothing else.  The plan is spectral_plan.cpp's.
#include "kernels_spectral.h"   // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

#include <vector>

struct lb_spectral {
    int nx = 0, ny = 0, device = 0;
    double lam = 1.0;
    SpPlan plan = {};
    cf *arr[3] = {nullptr, nullptr, nullptr};       // charge, xgrad, ygrad: [ny][nx]
    cf *tw[2] = {nullptr, nullptr};                 // twiddles of x and y
    hipStream_t stream = nullptr;                   // its own work; the coupled calls run on the lattice's stream (sp_borrow / sp_return)
    hipEvent_t ev = nullptr;
};

namespace {

SpDevAxis dev_axis(const SpAxis &a)
{
    SpDevAxis d = {a.n, a.npass, 0ull};
    for (int i = 0; i < a.npass; ++i) d.radices |= (unsigned long long)a.radix[i] << (4 * i);
    return d;
}

SpArgs sp_args(const lb_spectral *sp)
{
    SpArgs a = {};
    a.c = sp->arr[0]; a.x = sp->arr[1]; a.y = sp->arr[2];
    a.twx = sp->tw[0]; a.twy = sp->tw[1];
    a.nx = sp->nx; a.ny = sp->ny;
    a.rows = sp->plan.rows; a.cols = sp->plan.cols;
    a.lam2 = (float)(sp->lam * sp->lam);
    a.norm = (float)(1.0 / ((double)sp->nx * sp->ny));
    a.scale = 1.f;
    a.ax = dev_axis(sp->plan.x); a.ay = dev_axis(sp->plan.y);
    return a;
}

// the x-FFT of a.c's rows in place; real: of the plane a.real_in into a.c
int rows_fwd(const lb_spectral *sp, hipStream_t st, const SpArgs &a, bool real)
{
    const dim3 grid((unsigned)sp->plan.row_blocks), block(SP_THREADS);
    if (real) hipLaunchKernelGGL(k_sp_rows_fwd<true>, grid, block, (size_t)sp->plan.row_lds_bytes, st, a);
    else hipLaunchKernelGGL(k_sp_rows_fwd<false>, grid, block, (size_t)sp->plan.row_lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// the inverse x-FFT and 1 / (nx ny) of a.x (both: and of a.y) in place; vel: real parts x a.scale into a.u, a.v instead
int rows_inv(const lb_spectral *sp, hipStream_t st, const SpArgs &a, bool both, bool vel)
{
    const dim3 grid((unsigned)sp->plan.row_blocks, both ? 2u : 1u), block(SP_THREADS);
    if (vel) hipLaunchKernelGGL(k_sp_rows_inv<true>, grid, block, (size_t)sp->plan.row_lds_bytes, st, a);
    else hipLaunchKernelGGL(k_sp_rows_inv<false>, grid, block, (size_t)sp->plan.row_lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// mode 0 / 1: the forward / inverse y-FFT of a.c's columns in place; 2: k_sp_cols_mid
int cols(const lb_spectral *sp, hipStream_t st, const SpArgs &a, int mode)
{
    const dim3 grid((unsigned)sp->plan.col_blocks), block(SP_THREADS);
    const size_t lds = (size_t)sp->plan.col_lds_bytes;
    if (mode == 2) hipLaunchKernelGGL(k_sp_cols_mid, grid, block, lds, st, a);
    else if (mode == 1) hipLaunchKernelGGL(k_sp_cols<true>, grid, block, lds, st, a);
    else hipLaunchKernelGGL(k_sp_cols<false>, grid, block, lds, st, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int pointwise(const lb_spectral *sp, hipStream_t st, const SpArgs &a, bool grad)
{
    const dim3 grid((unsigned)(((long long)sp->nx * sp->ny + SP_THREADS - 1) / SP_THREADS)), block(SP_THREADS);
    if (grad) hipLaunchKernelGGL(k_sp_grad, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_sp_screen, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// the three fused launches on st; a.real_in != nullptr: the charge is that plane; vel: the gradients end as a.u, a.v
int solve_on(const lb_spectral *sp, hipStream_t st, const SpArgs &a, bool vel)
{
    int rc;
    if ((rc = rows_fwd(sp, st, a, a.real_in != nullptr))) return rc;
    if ((rc = cols(sp, st, a, 2))) return rc;
    return rows_inv(sp, st, a, true, vel);
}

SpArgs velocity_args(const lb_spectral *sp, const lb_sim *s, float scale)
{
    SpArgs a = sp_args(sp);
    a.real_in = s->rho; a.u = s->u; a.v = s->v;
    a.rpitch = (int)s->pitch;
    a.scale = scale;
    return a;
}

}  // namespace

// ---- what nutrient.cpp couples its set with (host.h) ---------------------------------------------------------------------------------
// the solver's arrays handed to another stream behind the solver's own work, and back
int sp_borrow(lb_spectral *sp, hipStream_t st)
{
    HIP_TRY(hipEventRecord(sp->ev, sp->stream));
    HIP_TRY(hipStreamWaitEvent(st, sp->ev, 0));
    return LB_OK;
}
int sp_return(lb_spectral *sp, hipStream_t st)
{
    HIP_TRY(hipEventRecord(sp->ev, st));
    HIP_TRY(hipStreamWaitEvent(sp->stream, sp->ev, 0));
    return LB_OK;
}

// what the coupled calls refuse, in the style of NEED_SCALAR
int sp_coupled_ready(const lb_spectral *sp, const lb_sim *s, const char *name)
{
    if (!sp) return fail(LB_ERR_ARG, "null spectral solver");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->cpu) return fail(LB_ERR_STATE, "%s is not available on the CPU backend", name);
    if (s->p.semantics != LB_SEM_DIFFUSION) return fail(LB_ERR_STATE, "%s is for scalar lattices (LB_SEM_DIFFUSION)", name);
    if (s->multi_slab()) return fail(LB_ERR_STATE, "%s is only available on a handle that owns the whole grid", name);
    if (s->p.nx != sp->nx || s->p.ny != sp->ny || s->p.device != sp->device)
        return fail(LB_ERR_ARG, "the lattice must have the spectral solver's grid (%d x %d) and device", sp->nx, sp->ny);
    if (s->stepping) return fail(LB_ERR_STATE, "%s inside a split step", name);
    return LB_OK;
}

// the three launches of the solve on s's stream: the charge is s's stored rho, u and v of s become scale x Re grad phi
int sp_velocity_on(const lb_spectral *sp, const lb_sim *s, float scale) { return solve_on(sp, s->stream, velocity_args(sp, s, scale), true); }

namespace {

#define NEED_SPECTRAL(sp)                                                        \
    do {                                                                         \
        if (!(sp)) return fail(LB_ERR_ARG, "null spectral solver");              \
    } while (0)
#define NEED_WHICH(which)                                                        \
    do {                                                                         \
        if ((which) < 0 || (which) > 2) return fail(LB_ERR_ARG, "which is LB_SPECTRAL_CHARGE, LB_SPECTRAL_XGRAD or LB_SPECTRAL_YGRAD"); \
    } while (0)

}  // namespace

extern "C" {

int lb_spectral_destroy(lb_spectral *sp)
{
    if (!sp) return LB_OK;
    DeviceGuard guard(sp->device);
    if (sp->stream) (void)hipStreamSynchronize(sp->stream);
    for (cf *p : sp->arr) if (p) (void)hipFree(p);
    for (cf *p : sp->tw) if (p) (void)hipFree(p);
    if (sp->ev) (void)hipEventDestroy(sp->ev);
    if (sp->stream) (void)hipStreamDestroy(sp->stream);
    delete sp;
    return LB_OK;
}

int lb_spectral_create(int nx, int ny, int device, double lam, lb_spectral **out)
{
    if (!out) return fail(LB_ERR_ARG, "null argument");
    *out = nullptr;
    SpPlan plan;
    if (!sp_plan(nx, ny, &plan)) return fail(LB_ERR_ARG, "a %d x %d grid: %s", nx, ny, sp_length_rule);
    if (!(lam >= 0.0) || !(lam <= 1.0e18)) return fail(LB_ERR_ARG, "the screening length must be finite and not negative");
    if (device < 0) return fail(LB_ERR_STATE, "lb_spectral_create is not available on the CPU backend");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return fail(LB_ERR_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    lb_spectral *sp = new lb_spectral;
    sp->nx = nx; sp->ny = ny; sp->device = device; sp->lam = lam; sp->plan = plan;
    const size_t bytes = sizeof(cf) * (size_t)nx * ny;
    hipError_t e = hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sp->ev, hipEventDisableTiming);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) {
        e = hipMalloc(&sp->arr[i], bytes);
        if (e == hipSuccess) e = hipMemsetAsync(sp->arr[i], 0, bytes, sp->stream);
    }
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        const int n = i ? ny : nx;
        std::vector<float> t(2 * (size_t)n);
        sp_twiddles(n, t.data());
        e = hipMalloc(&sp->tw[i], sizeof(cf) * (size_t)n);
        if (e == hipSuccess) e = hipMemcpy(sp->tw[i], t.data(), sizeof(cf) * (size_t)n, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(sp->stream);
    if (e != hipSuccess) {
        lb_spectral_destroy(sp);
        return fail(LB_ERR_HIP, "lb_spectral_create: %s", hipGetErrorString(e));
    }
    *out = sp;
    return LB_OK;
}

int lb_spectral_set_lambda(lb_spectral *sp, double lam)
{
    NEED_SPECTRAL(sp);
    if (!(lam >= 0.0) || !(lam <= 1.0e18)) return fail(LB_ERR_ARG, "the screening length must be finite and not negative");
    sp->lam = lam;
    return LB_OK;
}

int lb_spectral_set(lb_spectral *sp, int which, const float *re_im, int on_device)
{
    NEED_SPECTRAL(sp);
    NEED_WHICH(which);
    if (!re_im) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(sp->device);
    const size_t bytes = sizeof(cf) * (size_t)sp->nx * sp->ny;
    HIP_TRY(hipStreamSynchronize(sp->stream));
    HIP_TRY(hipMemcpy(sp->arr[which], re_im, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (on_device) HIP_TRY(hipDeviceSynchronize());
    return LB_OK;
}

int lb_spectral_get(lb_spectral *sp, int which, float *re_im)
{
    NEED_SPECTRAL(sp);
    NEED_WHICH(which);
    if (!re_im) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(sp->device);
    HIP_TRY(hipStreamSynchronize(sp->stream));
    HIP_TRY(hipMemcpy(re_im, sp->arr[which], sizeof(cf) * (size_t)sp->nx * sp->ny, hipMemcpyDeviceToHost));
    return LB_OK;
}

// forward: rows, then columns; inverse: columns, then rows and 1 / (nx ny) -- the order of the fused solve
int lb_spectral_transform(lb_spectral *sp, int which, int forward)
{
    NEED_SPECTRAL(sp);
    NEED_WHICH(which);
    DeviceGuard guard(sp->device);
    SpArgs a = sp_args(sp);
    a.c = a.x = sp->arr[which];
    int rc;
    if (forward) {
        if ((rc = rows_fwd(sp, sp->stream, a, false))) return rc;
        return cols(sp, sp->stream, a, 0);
    }
    if ((rc = cols(sp, sp->stream, a, 1))) return rc;
    return rows_inv(sp, sp->stream, a, false, false);
}

int lb_spectral_screen(lb_spectral *sp)
{
    NEED_SPECTRAL(sp);
    DeviceGuard guard(sp->device);
    return pointwise(sp, sp->stream, sp_args(sp), false);
}

int lb_spectral_grad_multiply(lb_spectral *sp)
{
    NEED_SPECTRAL(sp);
    DeviceGuard guard(sp->device);
    return pointwise(sp, sp->stream, sp_args(sp), true);
}

int lb_spectral_solve(lb_spectral *sp)
{
    NEED_SPECTRAL(sp);
    DeviceGuard guard(sp->device);
    return solve_on(sp, sp->stream, sp_args(sp), false);
}

int lb_spectral_velocity(lb_spectral *sp, lb_sim *s, float scale, int streamed)
{
    int rc = sp_coupled_ready(sp, s, "lb_spectral_velocity");
    if (rc) return rc;
    if (!finite32(scale)) return fail(LB_ERR_ARG, "the velocity's factor must be finite");
    DeviceGuard guard(s->p.device);
    if (streamed) rc = scalar_moments(s);
    else rc = ensure_macro(s);
    if (rc) return rc;
    if ((rc = sp_borrow(sp, s->stream))) return rc;
    if ((rc = solve_on(sp, s->stream, velocity_args(sp, s, scale), true))) return rc;
    s->feq_valid = false;
    return sp_return(sp, s->stream);
}

int lb_run_screened(lb_spectral *sp, lb_sim *s, float scale, int n_steps)
{
    int rc = sp_coupled_ready(sp, s, "lb_run_screened");
    if (rc) return rc;
    if (!finite32(scale)) return fail(LB_ERR_ARG, "the velocity's factor must be finite");
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    // (scalar_step would refuse this too, but only with the solver borrowed and rho, u, v of the first step written)
    if (s->noisy && s->ad_noise_field)
        return fail(LB_ERR_STATE, "lb_run_screened: a noise field is set (lb_set_noise_field): only lb_collide_particles uses one; drop it with NULL first");
    if (n_steps == 0) return LB_OK;
    DeviceGuard guard(s->p.device);
    if ((rc = sp_borrow(sp, s->stream))) return rc;
    const SpArgs a = velocity_args(sp, s, scale);
    for (int i = 0; i < n_steps; ++i) {
        if ((rc = scalar_moments(s))) return rc;
        if ((rc = solve_on(sp, s->stream, a, true))) return rc;
        if ((rc = scalar_step(s, i == n_steps - 1))) return rc;
    }
    s->feq_valid = false;
    s->macro_valid = true;
    return sp_return(sp, s->stream);
}

}  // extern "C"
