// host.h -- what the host-side translation units of liblbhip.so share: the handle, error reporting, the table of handle kinds, the RCCL
// entry points and the functions one unit offers the others.  Who holds what:
//   plan.cpp       the launch planner (plan.h): every decision that is arithmetic over PlanInputs; no HIP
//   launch.cpp     kernel arguments and launches of the fused flow kernels, hipGraph replay, a whole grid's run
//   slab.cpp       halo tables, pack / unpack, the exchanges, a slab's halo cycle and run, lb_run_group, lb_step_*, lb_halo_*
//   transport.cpp  the RCCL loader, lb_comm_*, lb_peer_*
//   tune.cpp       lb_autotune* and what they found, remembered (LB_TUNE_CACHE)
//   lb_hip.cpp     create / destroy / setters, state transfer, the entry points every kind shares (the un-fused phases, lb_run: common
//                  checks, then the kind's row), the flow kind's row, lb_run_batch, what set calls share (SetScope's join and release,
//                  set_fault), lb_check, timers
//   scalar.cpp, multifield.cpp, poisson.cpp, porous.cpp, multifluid.cpp, rocket.cpp
//                  one handle kind each: its kernels, their launches, its row of the kind table, its own entry points of the C ABI
//   spectral.cpp   the spectral screened-Poisson solver (lb_spectral_*: not a handle kind) and its coupling to a scalar lattice;
//                  spectral_plan.cpp its plan (spectral_plan.h): no HIP
//   nutrient.cpp   a population and its nutrient under the solver's velocity (lb_*_nutrient: two scalar lattices and an lb_spectral,
//                  no handle kind of its own); emits kernels_nutrient.h
//   expansion.cpp  noisy strains on a shared nutrient (lb_*_expansion: 2 ... 4 scalar lattices, no handle kind of its own); emits
//                  kernels_expansion.h
//   advected.cpp   a flow and the scalars it carries (lb_run_advected: one flow handle and 1 ... 2 scalar lattices, no handle kind of
//                  its own); emits kernels_advected.h
// Small kernels are emitted by the one unit that includes their header: kernels_phases.h + kernels_check.h by lb_hip.cpp,
// kernels_halo.h by slab.cpp, kernels_scalar.h by scalar.cpp (its health check's first pass only: check_reduce.h is shared, the folding
// pass is lb_hip.cpp's), kernels_multifield.h by multifield.cpp, kernels_poisson.h by poisson.cpp, kernels_porous.h by porous.cpp,
// kernels_multifluid.h by multifluid.cpp, kernels_rocket.h by rocket.cpp, kernels_spectral.h by spectral.cpp, kernels_nutrient.h by nutrient.cpp, kernels_expansion.h by expansion.cpp.  The six kind headers, kernels_nutrient.h and kernels_expansion.h share kernels_lane4.h, the plan their
// fused steps follow: device functions only, no kernel of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "../../include/lb_hip.h"
#include "cpu_backend.h"
#include "plan.h"
#include "launchers.h"          // StepArgs; the fused kernels are instantiated in their own translation units
#include "check_reduce.h"       // CheckPartial
#include "poisson_launch.h"     // PsState
#include "multifluid_launch.h"  // McInter, McReact; PmExtra (porous_launch.h)

namespace {

constexpr int MASK_GHOST = LB_MASK_HALO_ROWS;   // mask rows kept of each neighbouring slab (step 1 of row -13)
constexpr int GUARD = 512; // floats in front of / behind each lattice allocation (the marching kernels' last
                           // strip reads up to 257 cells past a row's end, every kernel 1 cell before its start)

}  // namespace

struct lb_sim : PlanInputs {
    lbcpu::CpuPipe *cpu = nullptr;   // device = LB_DEVICE_CPU: the host backend (cpu_backend.h); every device member below stays empty
    float *lat[2] = {nullptr, nullptr};   // raw allocations (with guards)
    int cur = 0;                // lattice holding f
    int stepping = 0;           // 1 between lb_step_boundary and lb_step_finish
    float *feq = nullptr;       // raw allocation, lazily created
    float *rho = nullptr, *u = nullptr, *v = nullptr;
    float *stage = nullptr;     // [H][pitch], lazily: one plane on its way between the host and interleaved rows (lattice_plane_*)
    float *ad_edge = nullptr;   // scalar lattice, OPEN family: the edge state on the device (scalar_launch.h: AdExtra)
    float ad_G = 0.f;           // scalar lattice: growth rate of the Fisher term (lb_set_reaction); 0 = plain relaxation
    float ad_Dg = 0.f;          // LB_SEM_DIFFUSION: strength of the noisy collision (lb_set_noise); 0 = the plain cell
    uint64_t ad_seed = 0, ad_t = 0;     // ... its stream's key and its noise counter: noisy collisions since the seed was set (philox.h)
    float *ad_noise_field = nullptr;    // ... a supplied [ny][nx] field of normals for lb_collide_particles (lb_set_noise_field), device
    float *vi_corner = nullptr; // VELOCITY_INLET: the eight corner links nothing ever writes (bc_vel_cell), device; LB_BC_BOX, LB_BC_DIRICHLET: likewise (MfBox, PsBox)
    // the LB Poisson solver (LB_SEM_POISSON; poisson_launch.h)
    float *ps_source = nullptr;         // [H][pitch]: the source, padding zero
    float *ps_part = nullptr;           // two floats per workgroup of k_ps_step
    PsState *ps_state = nullptr;        // the device's side of a solve: stop word, last ratio
    float ps_rho_b = 0.f, ps_react = 1.f, ps_tol = 1.0e-6f;     // lb_set_poisson
    int ps_iter = 0;                    // iterations since the last lb_solve_reset (solver.py's num_iterations)
    int ps_batch = 0;                   // lb_solve's launches between two reads of the stop word; 0 = PS_BATCH (LB_DIAG on such a handle: diagnosis)
    // forced flow in a porous medium (LB_SEM_POROUS; porous_launch.h)
    float *pm_G[2] = {nullptr, nullptr};    // [H][pitch] each: the total force of the last step
    float *pm_ub[2] = {nullptr, nullptr};   // [H][pitch] each: the barycentric velocity
    float *pm_field[2] = {nullptr, nullptr};    // [H][pitch] each, padding zero: the force field (lb_set_force_field), or none
    float pm_eps = 1.f, pm_nu = 0.f, pm_K = 1.f, pm_Fe = 0.f;   // lb_set_porous
    float pm_gx = 0.f, pm_gy = 0.f;         // lb_set_body_force
    // multicomponent Shan-Chen fluids (LB_SEM_MULTIFLUID; multifluid_launch.h): a member uses pm_G, pm_ub, pm_field, pm_gx, pm_gy as
    // the porous fluid does; the tables of a set live in its first handle
    McInter mc_inter[MC_MAX_INTER] = {};
    McReact mc_react[MC_MAX_REACT] = {};
    int mc_n_inter = 0, mc_n_react = 0;
    // surfactant-propelled colonies (LB_SEM_ROCKET; rocket_launch.h): the parameters of a set and what its last step left live in its
    // first handle -- pm_G the pseudo-force (FLOW) / the pressure force (FORCES), pm_ub the surface force, ry_op psi / S
    lb_rocket_params ry = {LB_ROCKET_FLOW, 0.f, 0.f, 0.f, 1.f, 0.f, 1.f, 1.f};
    float *ry_op = nullptr;     // [H][pitch]
    // (a scalar lattice that is the first of a clumpy nutrient set, nutrient.cpp, keeps psi in ry_op and F in pm_G, made at first use)
    uint8_t *mask_raw = nullptr, *mask = nullptr;   // [H+2*MASK_GHOST][pitch] + guards; mask -> row 0
    bool feq_valid = false;     // feq buffer consistent with rho,u,v
    bool macro_valid = true;    // rho,u,v hold the last step's fields (false: to be rebuilt from the populations, ensure_macro)
    CheckPartial *check_part = nullptr;     // lb_check's records (check_reduce.h): one per workgroup of the first pass + the folded result behind them
    long long check_cap = 0;                // ... and how many it holds
    hipStream_t own_stream = nullptr, stream = nullptr, comm_stream = nullptr, edge_stream = nullptr;
    hipEvent_t ev_boundary = nullptr, ev_interior = nullptr, ev_halo = nullptr, ev_packed = nullptr, ev_edge = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    // (ev_interior also orders a scalar lattice and the flow handle it takes its velocity from, lb_set_velocity_from: both are whole-grid
    //  handles there, whose runs never record it -- the slab schedules and lb_run_batch are its other users)
    ncclComm_t comm = nullptr;
    int rank = 0;               // (nranks: PlanInputs)
    float *halo_buf = nullptr;  // 4 x HALO_SEGS_DEEP (117) x nx floats: send north, send south, recv south, recv north (ensure_halo_buf)
    int ghost_depth = 0;        // ghost rows of lat[cur] hold this many of the neighbours' edge rows (0, 3, 6 or 8)
    hipGraph_t graph = nullptr;            // GRAPH_STEPS single-step launches, captured for small grids
    hipGraphExec_t graph_exec = nullptr;
    int graph_key = -1;                    // state the capture is valid for (cur, mask, variant)
    hipStream_t graph_stream = nullptr;
    bool graph_failed = false;
    // peer transport (lb_peer_export / lb_peer_connect): my flag block, the neighbours' flag blocks and lattices as mapped here
    unsigned long long *peer_flags = nullptr;
    bool peer_flags_fine = false;
    struct PeerNb {
        unsigned long long *flags = nullptr;
        float *lat_raw[2] = {nullptr, nullptr};     // base of the neighbour's allocations as mapped into this process
        bool mapped = false;                        // (opened through IPC: to be closed; false: the same process / shared with the other side)
        long long plane = 0, rowp = 0;
        int h = 0;
    } peer_nb[2];                                   // [0] = south, [1] = north
    unsigned long long peer_timeout_ticks = 0;
    int diag = 0;
    bool xchg_inline = false;   // slabs, split bands: the exchange on the COMPUTE stream, between the interior launches (lb_set_exchange_inline)
    // lb_exchange_timing: a pair of timing events around every halo exchange of lb_run, on the stream that carries it
    static constexpr int XT_RING = 256;
    bool xt_on = false;
    hipEvent_t xt_ev[2 * XT_RING] = {};
    int xt_count = 0, xt_dropped = 0;
    bool tune_cache_checked = false;    // LB_TUNE_CACHE has been consulted for this handle's present shape (lb_set_mask resets it)
    int64_t bytes = 0;

    float *origin(int which) const { return lat[which] + GUARD + GHOST * rowp; }   // plane 0, row 0, x 0
    float *feq_origin() const { return feq + GUARD + GHOST * rowp; }
    bool peer_connected() const { return transport == SLAB_PEER; }
};

#pragma GCC visibility push(hidden)         // (internal to the library: only lb_* is exported)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// records the message lb_last_error returns (this thread's); returns code.  (Every format is a literal the compiler checks against its
// arguments: build.py makes -Wformat and -Wformat-nonliteral errors.)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(LB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// Handles of the CPU backend: an entry point either has a host form or refuses.
#define CPU_UNSUPPORTED(s, name)                                                                            \
    do {                                                                                                    \
        if ((s) && (s)->cpu) return fail(LB_ERR_STATE, "%s is not available on the CPU backend", name);      \
    } while (0)

// Scalar lattices (LB_SEM_DIFFUSION, and the fields of a coupled set: LB_SEM_MULTIFIELD) are whole-grid handles without obstacles: what only slabs, masks or the flow kernels' tuning mean refuses.
// So are the porous-medium fluid (LB_SEM_POROUS) and the fluids of a multicomponent set (LB_SEM_MULTIFLUID), which are refused here under their own names.
#define SCALAR_UNSUPPORTED(s, name)                                                                         \
    do {                                                                                                    \
        NOT_ROCKET(s, name);                                                                                \
        if ((s) && (s)->scalar()) return fail(LB_ERR_STATE, "%s is not available on a scalar lattice (LB_SEM_DIFFUSION)", name); \
        NOT_POROUS(s, name);                                                                                \
    } while (0)
// A lattice of a surfactant-propelled colony (LB_SEM_ROCKET) is a scalar lattice that is refused under its own name, and by more calls:
// its velocity is the set's own, its collision needs both members.
#define ROCKET_REFUSED(name) fail(LB_ERR_STATE, "%s is not available on a lattice of a surfactant-propelled colony (LB_SEM_ROCKET)", name)
#define NOT_ROCKET(s, name)                                                                                 \
    do {                                                                                                    \
        if ((s) && (s)->rocket()) return ROCKET_REFUSED(name);                                              \
    } while (0)
#define NOT_POROUS(s, name)                                                                                 \
    do {                                                                                                    \
        if ((s) && (s)->porous()) return fail(LB_ERR_STATE, "%s is not available on a porous-medium fluid (LB_SEM_POROUS)", name); \
        if ((s) && (s)->multifluid()) return fail(LB_ERR_STATE, "%s is not available on a fluid of a multicomponent set (LB_SEM_MULTIFLUID)", name); \
    } while (0)

// ---- handle kinds -----------------------------------------------------------------------------------------------------------------
// What differs by the kind of a handle (its semantics), one row per kind; the three flow semantics share one.  The row is defined by the
// unit that holds the kind (flow: lb_hip.cpp); the entry points of lb_hip.cpp do their common checks and call through it.
struct KindOps {
    // What lb_create refuses before any device is touched, in this order: a family outside `families` ("<noun> takes <families_text>"),
    // a grid below 3x3 where every cell needs eight neighbours, a slab, the halo flag, the CPU backend.  noun == nullptr (flow): none
    // of this; lb_create's own rules for the flow semantics follow.
    const char *noun;
    unsigned families;              // bit b set: bc_mode b
    const char *families_text;
    bool eight_neighbours;
    bool before_exists;             // refused before (true) or after lb_create's "LB_BC_OPEN / LB_BC_BOX exists for ..." checks
    // lb_set_variant: -1 ... variant_max, else variant_text with variant_code (variant_text == nullptr: every word is taken)
    int variant_max;
    const char *variant_text;
    int variant_code;
    // nullptr: nothing to do (`pass` in the reference).  Called with the handle's device current and the common checks made.
    int (*create)(lb_sim *s);       // the kind's own buffers, on s->stream; lb_create destroys the handle if it fails
    int (*move_bcs)(lb_sim *s);
    int (*hydro)(lb_sim *s);
    int (*feq)(lb_sim *s);          // into s->feq_origin(), which exists
    int (*collide)(lb_sim *s);      // (collide_ready first, or the kind's refusal)
    int (*run)(lb_sim *s, int n_steps);
};
// (functions, not objects: a constant at namespace scope would be emitted into the device code of its unit as well)
const KindOps &kind_flow(), &kind_scalar(), &kind_multifield(), &kind_poisson(), &kind_porous(), &kind_multifluid(), &kind_rocket();
#define KIND_ROW(name, ...) const KindOps &name() { static const KindOps k = {__VA_ARGS__}; return k; }
const KindOps &kind_of(int semantics);          // (a semantics lb_create does not know: the flow row)
inline const KindOps &kind_of(const lb_sim *s) { return kind_of(s->p.semantics); }

// a HIP call inside a kind's create: the message lb_create reports, without a source line
#define CREATE_TRY(expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(LB_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- lb_hip.cpp ------------------------------------------------------------------------------------------------------------------
bool finite32(float x);                         // false for NaN and the infinities
int ensure_macro(lb_sim *s);                    // rho, u, v as of the last time step
int collide_ready(lb_sim *s);                   // lb_collide_particles: feq exists, rho, u, v are current
int copy_plane_h2d(lb_sim *s, float *dev, const float *host);   // host [rows][nx] <-> device [rows][pitch], on s->stream
int copy_plane_d2h(lb_sim *s, float *host, const float *dev);
int copy_quads(hipStream_t st, float *dst, const float *src, long long n4);     // k_copy4 over n4 aligned float4
// Set calls (lb_run_batch, lb_*_coupled, lb_*_fluids, lb_*_rocket, lb_*_nutrient, lb_*_expansion; lb_set_velocity_from with {flow,
// lattice}): the members checked, then everything enqueued on the first member's stream inside a SetScope.  The scope keeps the members'
// device current; join() puts the first member's stream behind whatever the others still have in flight, release() makes the others'
// streams see the result.  A call ends with `return sc.release();`.  One that leaves after a successful join without it -- a launch that
// failed -- is released by the destructor, which drops its own status and records no message: the failure that caused the return is the
// one reported.  (guard is the first member: the previous device comes back after the release.)
struct SetScope {
    DeviceGuard guard;
    lb_sim **f;
    int count;
    bool joined = false;
    SetScope(lb_sim **f_, int count_) : guard(f_[0]->p.device), f(f_), count(count_) {}
    SetScope(const SetScope &) = delete;
    ~SetScope();
    int join();
    int release();
};
// after a run of a set: feq is stale; rho, u, v are the last step's
inline void set_ran(lb_sim **f, int count)
{
    for (int i = 0; i < count; ++i) {
        f[i]->feq_valid = false;
        f[i]->macro_valid = true;
    }
}
// What the coupled, fluid, rocket and nutrient sets test member by member, in this order; set_fault names the first rule broken and the
// member (*at) that breaks it, the family's own *_members says it in the family's sentence.
enum SetFault { SET_FINE, SET_NULL_MEMBER, SET_ROCKET_NAMED, SET_KIND, SET_GEOMETRY, SET_SPLIT_STEP, SET_TWICE };
// rocket_named: a rocket handle is refused under its own name before its kind is looked at; split_checked: a member inside a split step is refused
SetFault set_fault(lb_sim **f, int count, int semantics, bool rocket_named, bool split_checked, int *at);
// what the members of such a set, and of an expansion, share: grid, boundary family, layout flag, device
inline bool same_geometry(const lb_sim *a, const lb_sim *b)
{
    return a->p.nx == b->p.nx && a->p.ny == b->p.ny && a->p.bc_mode == b->p.bc_mode && a->p.device == b->p.device &&
           (a->p.flags & LB_FLAG_PLANAR) == (b->p.flags & LB_FLAG_PLANAR);
}

// ---- transport.cpp: RCCL, loaded lazily so that single-GPU use never touches librccl ---------------------------------------------
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
extern Rccl g_rccl;
int rccl_load();

#define NCCL_TRY(expr)                                                                        \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail(LB_ERR_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));      \
    } while (0)

// ---- launch.cpp ------------------------------------------------------------------------------------------------------------------
StepArgs step_args(const lb_sim *s, int row_begin, int row_step, int row_count);
// the launch grids of the kinds' kernels over a whole grid: one thread per cell in workgroups of 256; 64 x 4 lanes of four cells each
inline dim3 cells_grid(const StepArgs &a) { return dim3((unsigned)((a.nx + 255) / 256), (unsigned)a.ny); }
inline dim3 step_grid(const StepArgs &a) { return dim3((unsigned)((a.fpitch / 4 + 63) / 64), (unsigned)((a.ny + 3) / 4)); }
// An un-fused phase of a whole-grid handle on its stream: k(step_args(s, 0, 1, H), more...) over grid x 256 threads -- one per cell
// (grid_cells) or, for the in-place boundary phases, one per cell of the longer edge (grid_edge)
inline dim3 grid_cells(const lb_sim *s) { return dim3((unsigned)((s->p.nx + 255) / 256), (unsigned)s->p.ny); }
inline dim3 grid_edge(const lb_sim *s) { return dim3((unsigned)((std::max(s->p.nx, s->p.ny) + 255) / 256)); }
template <typename K, typename... A>
int launch_phase(lb_sim *s, dim3 grid, K k, const A &...more)
{
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s->stream, step_args(s, 0, 1, s->H), more...);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}
// the single-step kernel over local rows row_begin + i*row_step, i < row_count
int launch_step(lb_sim *s, int row_begin, int row_step, int row_count, bool macro);
// A marching launch (k_step2 ... k_step5, k_deep: `depth` time steps per pass) over output rows [row_begin, row_end).
struct MarchRows {
    hipStream_t stream = nullptr;
    int row_begin = 0, row_end = 0;
    int depth = 2;
    bool macro = false;         // the rho, u, v epilogue
    MarchBands bands;           // edge bands: fixed segments; count == 0: one balanced round of resident waves (plan_march)
    int reserve = 0;            // wave slots left to a band launch running beside this one
};
int launch_marching(lb_sim *s, const MarchRows &r);
void drop_graph(lb_sim *s);
// n time steps on a whole-grid handle
int run_whole_grid(lb_sim *s, int n_steps, bool final_macro = true);

// ---- scalar.cpp ------------------------------------------------------------------------------------------------------------------
// the un-fused phases the coupled lattices and the colonies share with the scalar lattice: rho = sum f; feq from rho, u, v
int scalar_hydro(lb_sim *s);
int scalar_feq(lb_sim *s);
// what spectral.cpp steps a scalar lattice (LB_SEM_DIFFUSION) with: the density after streaming into s->rho, nothing moved
// (k_ad_moments); one k_ad_step with the velocity u, v hold now
int scalar_moments(lb_sim *s);
int scalar_step(lb_sim *s, bool store_rho);
// what advected.cpp's 1 + NS launch form steps a periodic, noiseless scalar lattice with: one k_ad_step on the FLOW's stream whose
// u, v are the flow handle's planes (no copy)
int scalar_step_carried(lb_sim *s, const lb_sim *flow, bool store_rho);
// OPEN: the edge state copied out of (k_ad_edge_capture) / patch: written back into (k_ad_edge_patch) the lattice at `f`
void lbk_ad_edge(bool patch, hipStream_t st, const StepArgs &a, float *f, float *edge);
// the health check's first pass over the lattice at a.src and the fields a.u, a.v: one record per workgroup, ad_check_blocks(a) of
// them, into part (k_check_final, lb_hip.cpp, folds them)
long long ad_check_blocks(const StepArgs &a);
void lbk_ad_check(hipStream_t st, const StepArgs &a, CheckPartial *part);

// ---- spectral.cpp: what a set coupled to the spectral solver (nutrient.cpp) runs it with ---------------------------------------------
struct lb_spectral;
int sp_borrow(lb_spectral *sp, hipStream_t st);     // the solver's arrays handed to another stream behind the solver's own work ...
int sp_return(lb_spectral *sp, hipStream_t st);     // ... and back
int sp_coupled_ready(const lb_spectral *sp, const lb_sim *s, const char *name);    // a whole-grid GPU scalar lattice of the solver's grid and device, or the refusal
int sp_velocity_on(const lb_spectral *sp, const lb_sim *s, float scale);           // the three launches on s's stream: s's stored rho -> s's u, v

// ---- porous.cpp: what a fluid of a multicomponent set shares with the porous-medium fluid (and a colony: the four planes) -------------
PmExtra pm_extra(const lb_sim *s);
int forced_create(lb_sim *s);                   // pm_G, pm_ub
int porous_move_bcs(lb_sim *s);
int porous_feq(lb_sim *s);

// ---- slab.cpp --------------------------------------------------------------------------------------------------------------------
int ensure_halo_buf(lb_sim *s);         // the send / receive buffers of the halo exchange (also lb_check's scratch across ranks)
int peer_check_error(lb_sim *s);
int run_slab(lb_sim *s, int n_steps);   // lb_run on a slab handle
extern const size_t peer_flag_bytes;    // a handle's flag block of the peer transport (kernels_halo.h)

// ---- tune.cpp --------------------------------------------------------------------------------------------------------------------
bool tune_cache_apply(lb_sim *s);       // takes over a remembered result (LB_TUNE_CACHE); true if the handle is tuned afterwards

#pragma GCC visibility pop
