// plan.h -- the launch planner: which kernel a handle runs, how many time steps a launch fuses, how a run of n steps is split into
// launches, how a marching launch is cut into strips and segments, how thick a slab's edge bands are.  Pure arithmetic over
// PlanInputs; plain C++ (no HIP, no RCCL), so a change here can be compiled and exercised on a host without a GPU.  Every rank of a
// multi-GPU run must take these decisions identically: PlanInputs is the list of what a decision may depend on.
#pragma once
#include "../../include/lb_hip.h"
#include "plan_consts.h"

#pragma GCC visibility push(hidden)         // (internal to the library: only lb_* is exported)

// what moves a slab's halo (deep2_chosen: the kernel of the seven-step cycle follows the transport)
enum SlabTransport : int { SLAB_NO_TRANSPORT = 0, SLAB_RCCL, SLAB_PEER };

// The plain-data part of a handle (lb_sim, host.h, derives from it).
struct PlanInputs {
    lb_params p;
    int H = 0;                  // rows owned
    long long pitch = 0, rowp = 0, plane = 0, lat_floats = 0;   // padded row width; lattice row / plane strides; floats per lattice
    bool has_mask = false;
    bool has_field = false;     // LB_SEM_POROUS: a force field is set (lb_set_force_field)
    bool noisy = false;         // LB_SEM_DIFFUSION: the noisy collision is on (lb_set_noise with Dg > 0)
    int cu_count = 256;
    int min_h = 0;              // smallest slab height over the ranks (every rank must pick the same schedule)
    int nranks = 1;             // slabs of the run (lb_comm_init / lb_peer_connect): with min_h, the tallest slab the run can hold
    int variant = -1;           // < 0: automatic (effective_variant), else an OR of LB_VAR_* (lb_variant_bits)
    int tuned_steps = 0;        // 0: not tuned; else the fused kernel depth (1..7) chosen by lb_autotune
    int tuned_wpc = 0;          // and its waves per CU for the marching kernels (-1: the LDS tiles)
    float depth_cost[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // ms per launch of the d-step kernel as lb_autotune timed it (0: not timed): launch_costs
    int forced_cycle = 0;       // slabs: depth of the fused kernel the halo cycle runs on, fixed by the caller (lb_set_slab_cycle); 0 = automatic
    int slab_flavour = -1;      // slabs, seven-step cycle: 0 k_deep<7>, 1 k_deep2<7> (lb_set_slab_cycle(8)), -1 automatic (k_deep2 under RCCL)
    int transport = SLAB_NO_TRANSPORT;   // slabs: lb_comm_init / lb_peer_connect

    bool multifield() const { return p.semantics == LB_SEM_MULTIFIELD; } // one field of a coupled set of scalar lattices (kernels_multifield.h)
    bool poisson() const { return p.semantics == LB_SEM_POISSON; }       // the LB Poisson solver (kernels_poisson.h)
    bool porous() const { return p.semantics == LB_SEM_POROUS; }         // forced flow in a porous medium (kernels_porous.h): a fluid, not scalar()
    bool multifluid() const { return p.semantics == LB_SEM_MULTIFLUID; } // one fluid of a set of Shan-Chen fluids (kernels_multifluid.h): a fluid, not scalar()
    bool rocket() const { return p.semantics == LB_SEM_ROCKET; }         // one lattice of a surfactant-propelled colony (kernels_rocket.h): a scalar lattice whose velocity the set computes
    bool scalar() const { return p.semantics == LB_SEM_DIFFUSION || multifield() || poisson() || rocket(); }  // a scalar lattice (kernels_scalar.h), on its own or coupled, or the Poisson solver's
    bool multi_slab() const { return H != p.ny || (p.flags & LB_FLAG_HALO); }
    int agreed_h() const { return min_h > 0 ? min_h : H; }      // the height all ranks decide on
};

// ---- which kernels -------------------------------------------------------------------------------------------------------------
int kernel_bc(const PlanInputs *s);
bool lazy_macro(const PlanInputs *s);
int effective_variant(const PlanInputs *s);
bool deep2_chosen(const PlanInputs *s);
bool marching_planes_fit(const PlanInputs *s);
// (h: the height the decision is taken on -- a slab's own, or the smallest of the slabs that must agree)
bool step2_applicable(const PlanInputs *s, int h = -1);
bool step3_applicable(const PlanInputs *s, int h = -1);
bool step4_applicable(const PlanInputs *s);
bool step5_applicable(const PlanInputs *s);
bool deep_applicable(const PlanInputs *s);
bool tile_applicable(const PlanInputs *s);
bool use_tile_kernel(const PlanInputs *s);
int tile_shape_of(const PlanInputs *s);
bool small_grid(const PlanInputs *s);
bool cython_tiles(const PlanInputs *s);
bool autotune_applies(const PlanInputs *s);
bool tune_entry_runs_here(const PlanInputs *s, int steps, int wpc);

// ---- how a run is split into launches -------------------------------------------------------------------------------------------
// sets of fused depths: bit d set = the d-step kernel may be used (bit 1 always is)
int depth_mask(bool two, bool three, bool four = false, bool five = false, bool six = false, bool seven = false);
int whole_grid_depths(const PlanInputs *s);
int slab_step_depths(const PlanInputs *s, int h);       // a slab outside its halo cycle: single, two and three steps
int cycle_depth(const PlanInputs *s, int h);
int next_advance(int allowed, int left, const float *cost);
void launch_costs(const PlanInputs *s, float (&cost)[MAX_DEPTH + 1]);
int next_advance(const PlanInputs *s, int allowed, int left);

// ---- the geometry of a marching launch ------------------------------------------------------------------------------------------
int march_strips(int nx, int depth);
// Output rows in `count` segments of `rows` rows spaced `stride` apart (edge bands); count == 0: cut into equal shares so that the
// launch is one balanced round of resident waves.
struct MarchBands { int count = 0, rows = 0, stride = 0; };
struct MarchPlan {
    int strips, segs, seg_rows;
    int seg_stride, edge_seg_rows;      // (StepArgs' fields of these names)
    int items;                          // workgroup items: strips x segs + the wall-column strips' extra ones
};
// rows: output rows of the launch; reserve: wave slots left to a concurrent band launch
MarchPlan plan_march(const PlanInputs *s, int rows, int depth, const MarchBands &bands, int reserve);
int band_extra(const PlanInputs *s, int D, bool split = false);

// ---- behind lb_steps_per_launch, lb_plan_launches, lb_hot_kernel (handles of the GPU backend) -------------------------------------
int steps_per_launch(const PlanInputs *s);
int plan_launches(const PlanInputs *s, int n_steps, int *depths, int max_launches);
void hot_kernel(const PlanInputs *s, char *buf, int buflen);
// scalar lattices: whether k_ad_tile4 takes the groups of four steps of a run (forced by the variant's LB_VAR_TILES, else by size),
// which of its three shapes, and the time steps of the next launch of a run with `left` steps to go: n = 4a + r as a tile
// launches, then r single steps (k_ad_step)
bool scalar_use_tiles(const PlanInputs *s);
// a set of Shan-Chen fluids (s = its first handle): the one-launch step k_mc_step, not k_mc_moments + k_mc_collide
bool multifluid_one_launch(const PlanInputs *s);
// a surfactant-propelled colony (s = its first handle): the one-launch step k_ry_step, not k_ry_moments + k_ry_collide
bool rocket_one_launch(const PlanInputs *s);
// a flow and the `count` scalars it carries (lb_run_advected) on a grid of `cells` cells: the form that runs for the caller's `form` (-1: the planner's)
int advected_form(long long cells, int count, int form);
int scalar_tile_shape(const PlanInputs *s);
int scalar_next_advance(const PlanInputs *s, int left);

#pragma GCC visibility pop
