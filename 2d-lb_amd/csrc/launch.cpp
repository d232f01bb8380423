// launch.cpp -- the launches of the fused flow kernels: their argument block (step_args: every kind's kernels take it), the single-step
// kernel, the marching kernels in the geometry the planner gives them (plan_march), the LDS tiles, hipGraph replay for small grids, the
// velocity-inlet family's band scheme, and a whole grid's run of n steps.  The kernels themselves are instantiated in the translation
// units of launchers.h.
#include "host.h"

StepArgs step_args(const lb_sim *s, int row_begin, int row_step, int row_count)
{
    StepArgs a;
    a.src = s->origin(s->cur);
    a.dst = s->origin(s->cur ^ 1);
    a.mask = s->has_mask ? s->mask : nullptr;
    a.rho = s->rho; a.u = s->u; a.v = s->v;
    a.plane = s->plane; a.pitch = (int)s->rowp; a.fpitch = (int)s->pitch;
    a.nx = s->p.nx; a.ny = s->p.ny; a.y0 = s->p.y0; a.h = s->H;
    a.row_begin = row_begin; a.row_step = row_step; a.row_count = row_count;
    a.wrap_y = (s->p.bc_mode == LB_BC_PERIODIC && !s->multi_slab()) ? 1 : (s->p.bc_mode == LB_BC_VELOCITY_INLET ? 2 : 0);
    a.u_w = s->p.inlet_u; a.u_e = s->p.outlet_u; a.corner = s->vi_corner;
    const bool periodic = (s->p.bc_mode == LB_BC_PERIODIC);
    a.ghost_s = (s->multi_slab() && (periodic || s->p.y0 > 0)) ? 1 : 0;
    a.ghost_n = (s->multi_slab() && (periodic || s->p.y0 + s->H < s->p.ny)) ? 1 : 0;
    a.seg_stride = 0;
    a.edge_seg_rows = 0;
    a.tile_launch_order = (s->variant >= 0 && (s->variant & LB_VAR_TILE_LAUNCH_ORDER)) ? 1 : 0;    // (A/B switch: explicit variants only)
    a.diag = s->diag;
    a.prio_turns = 0;      // (set by launch_marching from the variant)
    a.deep2_prio = 0;      // (set by launch_marching)
    a.nts = 0;
    a.omega = s->p.omega; a.rho_in = s->p.inlet_rho; a.rho_out = s->p.outlet_rho;
    a.lid_u = s->p.lid_u; a.rho0 = s->p.rho0;
    return a;
}

// Launch the fused step over local rows row_begin + i*row_step, i < row_count.
int launch_step(lb_sim *s, int row_begin, int row_step, int row_count, bool macro)
{
    if (row_count <= 0) return LB_OK;
    macro = macro && !lazy_macro(s);       // (no fused kernel stores rho, u, v on a handle that rebuilds them on demand)
    const StepArgs a = step_args(s, row_begin, row_step, row_count);
    const int variant = effective_variant(s);
    const int rpb_sel = variant & LB_VAR_ROWS;
    const int rows_per_block = rpb_sel == LB_VAR_ROWS_1 ? 1 : (rpb_sel == LB_VAR_ROWS_2 ? 2 : 4);
    const int waves_x = 4 / rows_per_block;          // waves side by side in x
    dim3 block(64 * waves_x, rows_per_block);
    const int lanes_x = (int)(s->pitch / 4);
    dim3 grid((lanes_x + block.x - 1) / block.x, (row_count + rows_per_block - 1) / rows_per_block);
    lbk_launch_step(kernel_bc(s), s->has_mask, macro, variant, grid, block, s->stream, a);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// A marching launch of `depth` time steps per pass (k_step2 ... k_step5, k_deep), by the translation unit that instantiates that depth.
// k_step4 gathers one row ahead where that fits in 256 registers without scratch (step4_prefetch, kernels_step4.h: every
// instantiation without an obstacle mask but the D2Q9i fork's); LB_VAR_STEP4_NO_AHEAD switches it off (A/B runs).
static bool launch_march(const lb_sim *s, hipStream_t st, const StepArgs &a, const MarchPlan &m, int row_end, bool macro, int depth)
{
    const int waves = (depth >= 4) ? STEP4_WAVES : 4;      // waves per workgroup: k_step4 ... k_step6: the two directions of ONE item
                                                           // (a segment pair); the others: four independent items
    MarchLaunch g;
    g.block = dim3(64, waves);
    g.grid = dim3(depth >= 4 ? m.items : (m.items + waves - 1) / waves);
    g.stream = st;
    g.strips = m.strips; g.seg_rows = m.seg_rows; g.nsegs = m.segs; g.row_end = row_end;
    const int bc = kernel_bc(s);
    // (false: the unit has no instantiation for this boundary family -- k_deep / k_deep2 and the velocity-inlet family)
    // k_deep2: four waves per workgroup -- asked for (LB_VAR_DEEP2) or found faster by lb_autotune (seven steps at "eight waves per CU")
    if (depth == 7 && deep2_chosen(s)) return lbk_launch_deep2_7(bc, s->has_mask, macro, g, a);
    if (depth == 7) return lbk_launch_deep7(bc, s->has_mask, macro, g, a);
    if (depth == 6) return lbk_launch_deep6(bc, s->has_mask, macro, g, a);
    if (depth == 5) lbk_launch_march5(bc, s->has_mask, macro, g, a);
    else if (depth == 4) lbk_launch_march4(bc, s->has_mask, macro, !(effective_variant(s) & LB_VAR_STEP4_NO_AHEAD), g, a);
    else lbk_launch_march23(depth, bc, s->has_mask, macro, g, a);
    return true;
}

// k_deep2: which role of a workgroup raises its issue priority at entry (kernels_deep2.h: deep2_set_prio): 0 none, 1 the front
// waves, 2 the back waves.  The front waves, since every shared SIMD holds a front and a back wave (roles by SIMD, kernels_deep2.h:
// deep2_take_role): a CU's two workgroups end together with either role raised, and the launch is 3-4 % shorter with the front
// waves -- four stages and the gather, the pace of their workgroup -- served first and the back waves on what they leave
// (profiles/deep2_roles_ab.txt; under the static roles it was the back waves: profiles/deep2_priority_ab.txt).  The diagnostic build
// overrides it per run (LB_DIAG bits 25-26).
constexpr int DEEP2_PRIO = 1;

int launch_marching(lb_sim *s, const MarchRows &r)
{
    if (r.row_end <= r.row_begin) return LB_OK;
    const bool macro = r.macro && !lazy_macro(s);
    StepArgs a = step_args(s, r.row_begin, 1, r.row_end - r.row_begin);
    const int variant = effective_variant(s);
    const MarchPlan m = plan_march(s, r.row_end - r.row_begin, r.depth, r.bands, r.reserve);
    a.seg_stride = m.seg_stride;
    a.edge_seg_rows = m.edge_seg_rows;
    // k_step4: the two waves of a SIMD take turns at the higher issue priority (see the kernel), in turns of 2^13 ticks of the 100 MHz clock; LB_VAR_NO_PRIO_TURNS = off
    a.prio_turns = (variant & LB_VAR_NO_PRIO_TURNS) ? 0 : 13;
    a.deep2_prio = DEEP2_PRIO;
    a.nts = (variant & LB_VAR_NT_STORES) ? 1 : 0;     // (the marching kernels take it at run time)
    if (!launch_march(s, r.stream, a, m, r.row_end, macro, r.depth))
        return fail(LB_ERR_STATE, "no %d-step kernel for this boundary family (the caller's schedule must not ask for one)", r.depth);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// Four time steps of a whole-grid handle through LDS tiles.
static int launch_tile4(lb_sim *s, bool macro)
{
    macro = macro && !lazy_macro(s);
    const StepArgs a = step_args(s, 0, 1, s->H);
    if (!lbk_launch_tile4(kernel_bc(s), s->has_mask, macro, tile_shape_of(s), s->p.nx, s->H, s->stream, a))
        return fail(LB_ERR_STATE, "no LDS-tile kernel for this boundary family");
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

constexpr int GRAPH_STEPS = 16;

void drop_graph(lb_sim *s)
{
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    s->graph_exec = nullptr;
    s->graph = nullptr;
    s->graph_key = -1;
}

// (Re)capture GRAPH_STEPS single-step launches starting from the current lattice.  The capture bakes in
// the lattice parity, the mask flag, the kernel variant and the stream, so it is redone when any changes.
// A capture failure is not an error: the caller falls back to eager launches.
static int ensure_graph(lb_sim *s)
{
    const int key = (s->cur & 1) | (s->has_mask ? 2 : 0) | (effective_variant(s) << 2);
    if (s->graph_exec && s->graph_key == key && s->graph_stream == s->stream) return LB_OK;
    if (s->graph_failed) return LB_OK;
    drop_graph(s);
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        s->graph_failed = true;
        return LB_OK;
    }
    int rc = LB_OK;
    const int cur0 = s->cur;
    for (int i = 0; i < GRAPH_STEPS && !rc; ++i) {
        rc = launch_step(s, 0, 1, s->H, false);
        s->cur ^= 1;
    }
    s->cur = cur0;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s->stream, &g);
    if (rc || e != hipSuccess || !g || hipGraphInstantiate(&s->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        s->graph_exec = nullptr;
        s->graph_failed = true;
        return LB_OK;
    }
    s->graph = g;
    s->graph_key = key;
    s->graph_stream = s->stream;
    return LB_OK;
}

// A d-step pass (d = 3, 4, 5) of the velocity-inlet family.  Rows [d, ny-d) depend on nothing the wall rows do within d steps:
// the marching kernel takes them, treating the wall rows as don't-care like any wall.  The 2d wall-side rows are advanced
// as a lattice of their own: the 2d rows next to each wall, stacked, ARE a velocity-inlet lattice of 4d rows -- row 0's pull
// reaches "row ny-2" = band row 4d-2, row ny-1's "row 1" = band row 1 -- except at the seam in the middle, whose garbage
// travels one row per step and after d steps has reached exactly the rows that are not needed.  One launch (k_vel_band:
// column chunks of the band in LDS, d steps there, the outer d + d rows stored) on the edge stream beside the interior's:
// both only read the current lattice and write disjoint rows of the other one.  (Round 2: the bands were copied into a
// second handle, stepped d times there and copied back -- a chain of a dozen small launches.)
static int vel_band_pass(lb_sim *s, int d, bool macro)
{
    int rc;
    const int H = s->H;
    const hipStream_t q = s->edge_stream;
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));          // everything enqueued so far (the previous pass included)
    HIP_TRY(hipStreamWaitEvent(q, s->ev_interior, 0));
    const StepArgs a = step_args(s, 0, 1, H);
    const dim3 grid((unsigned)((s->p.nx + (64 - 2 * d) - 1) / (64 - 2 * d))), blk(256);
    lbk_launch_vel_band(s->has_mask, macro, d, grid, blk, q, a);
    HIP_TRY(hipGetLastError());
    // the interior, from the same source lattice, on the compute stream
    MarchRows interior;
    interior.stream = s->stream; interior.row_begin = d; interior.row_end = H - d; interior.depth = d; interior.macro = macro;
    if ((rc = launch_marching(s, interior))) return rc;
    HIP_TRY(hipEventRecord(s->ev_boundary, q));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));   // the next pass (or the caller) sees the bands in place
    return LB_OK;
}

// n time steps on a whole-grid handle: largest fused kernel first in the remainder (n = 3a + rem with
// the three-step kernel, 2a + rem with the two-step kernel), hipGraph replay for small grids.
int run_whole_grid(lb_sim *s, int n_steps, bool final_macro)
{
    int rc;
    const int depths = whole_grid_depths(s);
    const bool tile = use_tile_kernel(s);
    int left = n_steps;
    // Small grids are launch-bound (a 256^2 step is ~3 us of GPU work against ~5 us of host launch
    // cost): replay GRAPH_STEPS single-step launches captured once into a hipGraph.
    if (depths == depth_mask(false, false) && left > GRAPH_STEPS && small_grid(s)) {
        if ((rc = ensure_graph(s))) return rc;
        while (s->graph_exec && left > GRAPH_STEPS) {          // keep >= 1 step for the MACRO launch
            HIP_TRY(hipGraphLaunch(s->graph_exec, s->stream));
            left -= GRAPH_STEPS;                                // GRAPH_STEPS is even: cur is unchanged
        }
    }
    const bool store_macro = final_macro && !lazy_macro(s);   // (lazy: rebuilt from the populations when asked for)
    while (left > 0) {
        const int adv = next_advance(s, depths, left);
        const bool macro = store_macro && (left == adv);
        if (adv == 4 && tile) rc = launch_tile4(s, macro);
        else if (adv >= 3 && s->p.bc_mode == LB_BC_VELOCITY_INLET) rc = vel_band_pass(s, adv, macro);
        else if (adv >= 2) {
            MarchRows all;
            all.stream = s->stream; all.row_begin = 0; all.row_end = s->H; all.depth = adv; all.macro = macro;
            rc = launch_marching(s, all);
        }
        else rc = launch_step(s, 0, 1, s->H, macro);
        if (rc) return rc;
        s->cur ^= 1;
        left -= adv;
    }
    if (n_steps) {
        s->feq_valid = false;
        // only a family whose fields are rebuilt on demand is ever flagged for a rebuild (see ensure_macro); a tuning pass
        // (final_macro = false) on the others leaves the fields of an earlier step in place until its closing MACRO step
        s->macro_valid = store_macro || !lazy_macro(s) || (s->diag & 4096);      // (LB_DIAG bit 12: the rho array carries the diagnostic build's per-wave timeline)
    }
    return LB_OK;
}
