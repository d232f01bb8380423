// poisson.cpp -- the LB Poisson solver (LB_SEM_POISSON): the kernels of kernels_poisson.h and their launches, the kind's row of the kind
// table (host.h: KindOps), its run, and the entry points of the C ABI that are its own: lb_set_poisson ... lb_solve, lb_gradient.
#include "kernels_poisson.h"    // (first: host.h switches floating-point contraction off for what follows it, cpu_backend.h)
#include "host.h"

namespace {

// The fused iteration over the whole grid.  solve: the form lb_solve enqueues -- returns at once when the stop word is set, stores rho
// and leaves its workgroup's two sums in e.part; !solve: lb_run's -- no stop word, no sums, rho when e.store_rho
void ps_step(bool solve, hipStream_t st, const StepArgs &a, const PsExtra &e)
{
    const dim3 block(64, 4), grid = step_grid(a);
    if (solve) hipLaunchKernelGGL(k_ps_step<true>, grid, block, 0, st, a, e);
    else hipLaunchKernelGGL(k_ps_step<false>, grid, block, 0, st, a, e);
}

PsExtra ps_extra(const lb_sim *s)
{
    const float w0 = 4.f / 9.f;
    return PsExtra{s->ps_source, s->ps_part, s->ps_state, (-1.f + w0) * s->ps_rho_b, s->ps_react, 0};
}

int poisson_create(lb_sim *s)
{
    // (the diagnostic word of the flow kernels means nothing here: on this handle it is lb_solve's batch length)
    s->ps_batch = s->diag > 0 ? s->diag : 0;
    s->diag = 0;
    const size_t fld_bytes = sizeof(float) * s->pitch * s->H;
    const size_t part_bytes = 2 * sizeof(float) * (size_t)ps_step_blocks(step_args(s, 0, 1, s->H));
    CREATE_TRY(hipMalloc(&s->ps_source, fld_bytes));
    CREATE_TRY(hipMemsetAsync(s->ps_source, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMalloc(&s->ps_part, part_bytes));
    CREATE_TRY(hipMemsetAsync(s->ps_part, 0, part_bytes, s->stream));
    CREATE_TRY(hipMalloc(&s->ps_state, sizeof(PsState)));
    const PsState fresh = {0, nanf(""), 0, 0};
    CREATE_TRY(hipMemcpy(s->ps_state, &fresh, sizeof(fresh), hipMemcpyHostToDevice));
    s->bytes += fld_bytes + part_bytes + sizeof(PsState);
    return LB_OK;
}

// The un-fused phases (lb_move is k_move + copy).  D2Q9_poisson.cl's move_bcs: the prescribed value on four walls, in place (edge cells only)
int poisson_move_bcs(lb_sim *s) { return launch_phase(s, grid_edge(s), k_ps_move_bcs, s->origin(s->cur), ps_extra(s).wall); }
int poisson_hydro(lb_sim *s) { return launch_phase(s, grid_cells(s), k_ps_hydro); }      // rho = (9/5)(f1 + ... + f8)
int poisson_feq(lb_sim *s) { return launch_phase(s, grid_cells(s), k_ps_feq, s->feq_origin()); }

// f relaxed in place towards feq, plus the source term
int poisson_collide(lb_sim *s)
{
    int rc = collide_ready(s);
    return rc ? rc : launch_phase(s, grid_cells(s), k_ps_collide, s->origin(s->cur), s->feq_origin(), s->ps_source, s->ps_react);
}

// n iterations in lb_run's form: k_ps_step<false>, one launch each, no stop word, no sums; the last launch stores rho, which is the
// next iteration's rho_before.  They count as iterations of the solve (solver.py:346).
int run_poisson(lb_sim *s, int n_steps)
{
    PsExtra e = ps_extra(s);
    for (int it = 0; it < n_steps; ++it) {
        e.store_rho = it == n_steps - 1;
        ps_step(false, s->stream, step_args(s, 0, 1, s->H), e);
        HIP_TRY(hipGetLastError());
        s->cur ^= 1;
    }
    s->ps_iter += n_steps;
    if (n_steps) { s->feq_valid = false; s->macro_valid = true; }
    return LB_OK;
}

// lb_solve's launches between two reads of the stop word.  profiles/poisson_bench.txt: the read-back is one host round trip per batch,
// the launches behind a stop inside a batch are empty early-outs.
const int PS_BATCH = 32;

}  // namespace

long long ps_step_blocks(const StepArgs &a)
{
    const dim3 g = step_grid(a);
    return (long long)g.x * g.y;
}

KIND_ROW(kind_poisson,
    "the LB Poisson solver (LB_SEM_POISSON)", 1u << LB_BC_DIRICHLET, "the family LB_BC_DIRICHLET only", false, true,
    0, "the LB Poisson solver (LB_SEM_POISSON) takes the variants -1 and 0 only: k_ps_step, no tiles", LB_ERR_STATE,
    poisson_create, poisson_move_bcs, poisson_hydro, poisson_feq, poisson_collide, run_poisson)

#define NEED_POISSON(s, name)                                                                                \
    do {                                                                                                     \
        if (!(s)) return fail(LB_ERR_ARG, "null handle");                                                    \
        NOT_POROUS(s, name);                                                                                 \
        NOT_ROCKET(s, name);                                                                                 \
        if (!(s)->poisson()) return fail(LB_ERR_STATE, "%s is for the LB Poisson solver (LB_SEM_POISSON)", name); \
    } while (0)

extern "C" {

int lb_set_poisson(lb_sim *s, float rho_on_boundary, float react_factor, float tolerance)
{
    NEED_POISSON(s, "lb_set_poisson");
    if (!finite32(rho_on_boundary) || !finite32(react_factor)) return fail(LB_ERR_ARG, "rho_on_boundary and react_factor must be finite");
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
            ps_step(true, s->stream, step_args(s, 0, 1, s->H), e);
            HIP_TRY(hipGetLastError());
            s->cur ^= 1;
            if (it >= 2) {
                // folds the partials of the k_ps_step in front of it (float64, fixed order), stores the ratio and, if the ratio is
                // < tolerance (false for inf and NaN), writes `it` into the stop word; returns at once when the stop word is set
                hipLaunchKernelGGL(k_ps_check, dim3(1), dim3(PS_CHECK_THREADS), 0, s->stream, (const float *)s->ps_part, blocks, s->ps_state, it, s->ps_tol);
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

// One launch into the handle's u, v planes (central differences of rho over the box, 0 for a neighbour outside) -- which no other kernel
// of this semantics writes: they hold the last gradient, lb_get_macro returns it --, then one pitched copy each to wherever the caller's
// pointers lead.
int lb_gradient(lb_sim *s, float inv_two_dx, float *ddx, float *ddy)
{
    NEED_POISSON(s, "lb_gradient");
    if (!finite32(inv_two_dx)) return fail(LB_ERR_ARG, "inv_two_dx must be finite");
    DeviceGuard guard(s->p.device);
    int rc = launch_phase(s, grid_cells(s), k_ps_gradient, inv_two_dx);
    if (rc) return rc;
    float *out[2] = {ddx, ddy};
    const float *from[2] = {s->u, s->v};
    for (int i = 0; i < 2; ++i)
        if (out[i])
            HIP_TRY(hipMemcpy2DAsync(out[i], s->p.nx * sizeof(float), from[i], s->pitch * sizeof(float), s->p.nx * sizeof(float), s->H,
                                     hipMemcpyDefault, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

}  // extern "C"
