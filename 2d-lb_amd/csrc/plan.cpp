// plan.cpp -- the launch planner (plan.h): host arithmetic only.  The thresholds below are measurements; the comments beside them
// say which, and name the files under profiles/ that hold them.  tests/plan_props.cpp sweeps what this file promises on a host (every
// row of every strip marched once, one round of wave slots, the ranks' agreement ...): a change to the item table runs it first.
#include "plan.h"

#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// boundary family as the kernels' template argument (the D2Q9i fork is the PIPE family with its own cell routines)
int kernel_bc(const PlanInputs *s) { return s->p.semantics == LB_SEM_OPENCL_D2Q9I ? LB_BC_PIPE_I : s->p.bc_mode; }

// rho, u, v of the plain families are rebuilt from the populations on demand instead of being stored by the last launch
// of every run (include/lb_hip.h, LB_FLAG_EAGER_MACRO); LB_EAGER_MACRO=1 in the environment = the flag on every handle
bool lazy_macro(const PlanInputs *s)
{
    static const bool eager_env = getenv("LB_EAGER_MACRO") && atoi(getenv("LB_EAGER_MACRO")) != 0;
    return !eager_env && !(s->p.flags & LB_FLAG_EAGER_MACRO) && s->p.semantics == LB_SEM_OPENCL &&
           (s->p.bc_mode == LB_BC_PIPE || s->p.bc_mode == LB_BC_PERIODIC || s->p.bc_mode == LB_BC_CAVITY);
}

// The variant word in use: lb_variant_bits (LB_VAR_*, include/lb_hip.h).  variant < 0 = automatic, from one-GPU sweeps (tools/sweep.py, tools/rect_probe.py;
// profiles/r01_sweep_variants.txt):
//   >= 1024^2 / 1280^2 cells on this GPU : temporal blocking -- three / four time steps per pass (marching
//                                          kernels; nx >= 512 and enough rows, else they do not apply)
//   lattice pair >= 450 MB (3072^2 up)   : + non-temporal stores (+3..10 %), and 4 rows x 256 cells per
//                                          workgroup wherever the single-step kernel runs (with contiguous
//                                          planes 2 x 512 was the better shape; with interleaved rows 4 x 256
//                                          streams 3..8 % faster at 4096^2 / 8192^2: profiles/r02_experiments.txt)
//   smaller (Infinity-Cache resident)    : single step, plain stores, XCD-aware tile order
int effective_variant(const PlanInputs *s)
{
    if (s->variant >= 0) return s->variant;
    const double pair_bytes = 2.0 * sizeof(float) * (double)s->lat_floats;
    const double cells = (double)s->p.nx * (s->min_h > 0 ? s->min_h : s->H);   // (ranks of one run agree on min_h)
    // non-temporal stores from ~450 MB per lattice pair (round 3), i.e. once the pair no longer fits the 256 MB Infinity Cache with room
    // to spare (round 3, k_step4, plain vs non-temporal: 311 MB 235.8 / 235.5 k MLUPS, 302 MB 232 / 227 k, 604 MB 241 / 265 k,
    // 613 MB 247 / 273 k -- the slab of one of eight GPUs at 8192^2 --, 680 MB 255 / 257 k, 1.2 GB 278 / 294 k:
    // profiles/r03_experiments.txt; the threshold was 1 GB)
    // (round 6, the deep kernels, plain | non-temporal, k MLUPS, profiles/r06l_nt_stores_midsize.txt, r06l_reference_case_bits.txt: pair of
    //  170 MB (periodic 1536^2) 306 | 298, 302 MB (2048^2) 369 | 363, pipe 2048^2 291 | 295; 338 MB -- the reference's 3751 x 1251 case --
    //  274-285 | 292-293 (two rounds, both depths), 415 MB: periodic 2400^2 385 | 388, pipe 337 against 308, cavity + mask 298 against 276:
    //  the threshold is 320 MB now)
    int v = pair_bytes >= 3.2e8 ? ((s->p.flags & LB_FLAG_PLANAR) ? LB_VAR_NT_STORES | LB_VAR_ROWS_2 : LB_VAR_NT_STORES) : LB_VAR_XCD_ORDER;
    // from 1024^2 cells: three steps per pass (110 k MLUPS at 1024^2 against 87 k single-step); from 1280^2:
    // four (125 k at 1280^2, 158 k at 1536^2, 170 k at 2048^2, 220 k from 3072^2), whole grids and slabs alike,
    // in every boundary family, with and without obstacles (profiles/r01_sweep_variants.txt,
    // profiles/r01_slab_proxy_1gpu.txt).  Smaller grids: single step, replayed through a hipGraph.
    if (cells >= 1024.0 * 1024.0) v = (v & ~LB_VAR_XCD_ORDER) | LB_VAR_STEP2 | LB_VAR_STEP3;
    if (cells >= 1280.0 * 1280.0) v |= LB_VAR_STEP4;
    // ... and five wherever four are (k_step5, overlapping strips: periodic 2048^2 298 against 250 k MLUPS, 4096^2 315 against 289 k,
    // 8192^2 327-346 against 306-319 k; pipe 8192^2 346 against 309 k: profiles/r04_experiments.txt section 10), in every family,
    // whole grids and slabs (cycle_depth) alike
    if (cells >= 1280.0 * 1280.0) v |= LB_VAR_STEP5;
    // ... and six / seven (k_deep, round 5: ONE wave per SIMD with the next row's gather in flight; kernels_deep.h) on the large whole
    // grids.  k MLUPS, k_step5 / k_deep<6> / k_deep<7>, one box (profiles/r05_size_sweep.txt): periodic 2048^2 281 / 283 / 279,
    // 2560^2 282 / 290 / 302, 4096^2 314 / 345 / 358, 8192^2 342 / 411 / 432 (other boxes: 346 / 436 / 459); pipe 3072^2 280 / 252 / 255,
    // 4096^2 303 / 318 / 323, 6144^2 303 / 370 / 371, 8192^2 333 / 387 / 394; cavity 4096^2 324 / 319 / 322, 6144^2 303 / 368 / 366;
    // with a (dense, random 1 %) obstacle mask -- 32 selects per row and stage that a lone wave pays in full --: periodic 2560^2
    // 254 / 244 / 261, 8192^2 338 / 347 / 368; pipe 4096^2 293 / 270 / 280, 6144^2 295 / 298 / 321; cavity 6144^2 321 / 305 / 322.
    // With the gathered row waited for by hand (kernels_deep.h, deep_row_issue; profiles/r05_size_sweep2.txt, another box): periodic
    // 1536^2 253 / 252 / 263, 2048^2 279 / 309 / 307, 3072^2 290 / 314 / 327; with a mask 1536^2 229 / 236 / 248, 2560^2 272 / 256 / 292;
    // pipe 3584^2 296 / 277 / 288, 4096^2 310 / 318 / 329; cavity 3584^2 296 / 299 / 301; pipe + mask 3584^2 280 / 259 / 264, 4096^2
    // 291 / 293 / 298 (config 5's image: 297 / 296 / 307), 5120^2 282 / 327 / 335; cavity + mask 4096^2 292 / 302 / 309.  Whole grids
    // from 1500^2 (periodic) cells -- the walled families: below --; slabs (edge bands of a deep cycle on few rows: section 9
    // of profiles/r05_experiments.txt) keep the thresholds they were measured with.
    const bool periodic_box = s->p.bc_mode == LB_BC_PERIODIC;
    const bool whole_grid = s->H >= s->p.ny;
    // Third sweep, after the wall-strip split had been repaired (its search window missed the optimum at these sizes: section 25 of the
    // log) and the wall strips' cost re-scanned (2.1): k_step5 | k_deep<6> | k_deep<7>, profiles/r05_size_sweep3.txt / r05_size_sweep4.txt:
    // pipe 2048^2 245 | 249 | 252, 2304^2 259 | 254 | 261, 2560^2 259 | 273 | 282, 3072^2 287 | 309 | 317, 3584^2 297 | 334 | 344; cavity
    // likewise; with a mask: pipe 2304^2 231 | 230 | 235, 2560^2 239 | 245 | 254, 3072^2 271 | 277 | 283, 3584^2 281 | 298 | 304; cavity 2304^2
    // 247 | 229 | 234, 2560^2 243 | 248 | 253; the reference's published case, 3751 x 1251 pipe + disc (4.69 M cells, 16 strips of short
    // segments): 231-233 | 242-244 | 251 (profiles/r05_refcase_kernels.txt).  Walled whole grids from 2300^2, with a mask from 2150^2 cells
    // -- just below the reference case, which gains 8 %; a square cavity with a dense mask between 2150^2 and 2500^2 loses up to 5 % --
    // (slabs: as measured before).
    // (slabs: ONE threshold per family, mask or not -- the halo cycle's depth follows from this choice (cycle_depth), every rank of a
    //  run must arrive at the same one, and the ranks agree on nx, min_h and the family but not on who holds obstacle cells: with
    //  round 5's 3800^2 / 4000^2 a rank with a mask and a rank without could pick different cycles between the two sizes)
    // Round 6, after the relaxation's fold, the non-temporal threshold above and k_deep2 (the seven steps by two waves per strip and
    // direction, two per SIMD -- short segments and wall columns are where a second wave per SIMD pays): k_step5 | k_deep<7> | k_deep2<7>,
    // k MLUPS, one box (profiles/r06o_walled_small_sweep.txt): pipe 1536^2 228 | 208 | 221, 1792^2 252 | 269 | 280, 2048^2 270 | 294 | 302,
    // 2304^2 286 | 316 | 323, 2560^2 283 | 342 | 345; cavity 1792^2 264 | 266 | 290, 2048^2 284 | 292 | 315, 2560^2 288 | 341 | 354; pipe + mask
    // 1792^2 233 | 236 | 249, 2048^2 255 | 255 | 270, 2560^2 273 | 300 | 310; the reference's case (2166^2 cells) 277 | 293 | 300; periodic with
    // a mask 1280^2 220 | 239 | 225, 1536^2 268 | 287 | 273, 2048^2 280 | 341 | 336.  lb_autotune (profiles/r06n_tune_probe.txt): pipe from
    // 3072^2 k_deep<7>, cavity k_deep2 up to 8192^2 within 1 % of k_deep.  Hence, whole grids: walled from 1700^2 cells, by k_deep2 below
    // 2900^2; periodic with a mask from 1250^2.  (Slabs: as measured before.)
    const double deep_side = periodic_box ? (whole_grid ? (s->has_mask ? 1250.0 : 1500.0) : 2400.0)
                                          : (whole_grid ? 1700.0 : 3800.0);
    // (not the velocity-inlet family: its wall-row bands stop at five steps and k_deep has no instantiation for it)
    if (cells >= deep_side * deep_side && s->p.bc_mode != LB_BC_VELOCITY_INLET) {
        v |= LB_VAR_STEP6 | LB_VAR_STEP7;     // (slabs: inside the twelve- / fourteen-step halo cycle, cycle_depth)
        if (whole_grid && !s->multi_slab() && !periodic_box && cells < 2900.0 * 2900.0) v |= LB_VAR_DEEP2;
    }
    // Periodic whole grids without a mask, tiles | k_step5 | k_deep<6> | k_deep<7>, k MLUPS, 1680-step runs (profiles/r06q_periodic_small_sweep.txt):
    // 1024^2 214 | 186 | 205 | 195, 1152^2 220 | 227 | 246 | 239, 1280^2 234 | 256 | 263 | 258, 1408^2 242 | 266 | 291 | 287, 1536^2 245 | 291 | 310 | 308,
    // 1792^2 254 | 319 | 364 | 359, 2048^2 210 | 293 | 340 | 364: six steps per pass from 1100^2 cells, seven from 1900^2 (use_tile_kernel:
    // the tiles below 1100^2).
    if (periodic_box && whole_grid && !s->multi_slab() && !s->has_mask) {
        v &= ~(LB_VAR_STEP6 | LB_VAR_STEP7);
        if (cells >= 1100.0 * 1100.0) v |= LB_VAR_STEP4 | LB_VAR_STEP5 | LB_VAR_STEP6;
        if (cells >= 1900.0 * 1900.0) v |= LB_VAR_STEP7;
    }
    return v;
}

// the seven steps of a pass by k_deep2<7> (four waves per workgroup) instead of k_deep<7>
bool deep2_chosen(const PlanInputs *s)
{
    if (s->multi_slab() && s->slab_flavour >= 0) return s->slab_flavour == 1;      // lb_set_slab_cycle(7) / (8): the caller's word
    if (s->variant >= 0) return (s->variant & LB_VAR_DEEP2) != 0;
    // Slabs without the caller's word (above: the ranks' collective tuner): by transport.  Beside k_deep<7> (2 x 80 KB of
    // LDS per CU, lone waves) RCCL's send / receive kernel waits for places and slows what it shares SIMDs with; k_deep2<7>'s launches
    // (2 x 72 KB, waves in pairs per SIMD) do not run longer for it, though it still takes most of a launch beside them: one slab of 4 | 2 of an 8192^2 lattice over RCCL 381-392 | 402-450 k MLUPS by k_deep, 443-444 | 466 k by
    // k_deep2 = the peer transport's rate; of 8: 374-381 | 383-392; the peer transport itself: equal within 1 %
    // (profiles/r06s_slab_proxy_deep2.txt).  Every rank of a run shares the transport, so the ranks agree.
    if (s->multi_slab()) return s->transport == SLAB_RCCL;
    if (s->tuned_steps) return s->tuned_steps == 7 && s->tuned_wpc == 8;       // lb_autotune's word
    return (effective_variant(s) & LB_VAR_DEEP2) != 0;                                // the size table's
}

// The marching kernels address the nine planes of a row through ONE scalar base and a 32-bit byte offset per lane that carries the
// plane (store_row9): (x + 8 plane) * 4 must stay below 4 GB.  Always true for the default layout (plane = the padded row);
// LB_FLAG_PLANAR lattices of more than ~11000^2 cells take the single-step kernel and the tiles instead.
// (Slabs: the halo cycle's depth hangs on this, and every rank of a run must arrive at the same one.  The plane stride of an
//  LB_FLAG_PLANAR slab grows with its OWN height, so a tall slab beside a short one -- 11264 and 1024 rows of 12288^2 -- found
//  its planes too far apart and dropped the cycle its neighbour kept.  The ranks agree on ny, min_h and their number: each decides on
//  the tallest slab such a run can hold, ny - (nranks - 1) min_h rows, which is at least its own -- and its own where the rows are
//  shared out evenly.  An uneven run whose tallest slab could be too tall, though none is, takes single steps: the price of
//  agreeing without a further exchange.)
bool marching_planes_fit(const PlanInputs *s)
{
    double plane = (double)s->plane;
    if (s->multi_slab() && (s->p.flags & LB_FLAG_PLANAR) && s->min_h > 0 && s->nranks > 1)
        plane = (double)(std::max(s->H, s->p.ny - (s->nranks - 1) * s->min_h) + 2 * GHOST) * (double)s->pitch;
    return (8.0 * plane + (double)s->rowp) * 4.0 < 4294967296.0;
}

bool step3_applicable(const PlanInputs *s, int h)
{
    if (h < 0) h = s->H;
    if (!marching_planes_fit(s)) return false;
    if (s->p.nx < 512 || h < (s->multi_slab() ? 32 : 128)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// four steps per pass on a whole-grid handle (slabs use it inside the eight-step halo cycle only: cycle_depth)
bool step4_applicable(const PlanInputs *s)
{
    if (s->multi_slab() || s->p.nx < 512 || s->H < 128 || !marching_planes_fit(s)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// five steps per pass (k_step5) on a whole-grid handle (slabs: inside the ten-step halo cycle, cycle_depth)
bool step5_applicable(const PlanInputs *s) { return step4_applicable(s); }
// six / seven steps per pass (k_deep): whole-grid handles; not the velocity-inlet family (its wall-row bands stop at five)
bool deep_applicable(const PlanInputs *s) { return step4_applicable(s) && s->p.bc_mode != LB_BC_VELOCITY_INLET; }

// four steps per pass through LDS tiles (k_tile4): whole-grid handles, any width
bool tile_applicable(const PlanInputs *s)
{
    return s->p.bc_mode != LB_BC_VELOCITY_INLET && !s->multi_slab() &&
           s->p.nx >= 64 && s->H >= 64;
}

bool step2_applicable(const PlanInputs *s, int h)
{
    if (h < 0) h = s->H;
    if (s->p.nx < 512 || !marching_planes_fit(s)) return false;
    if (h < (s->multi_slab() ? 16 : 64)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// strips a marching launch of `depth` steps per pass cuts nx columns into (k_step5, k_deep: overlapping strips, 248 / 240 cells apart)
int march_strips(int nx, int depth)
{
    return depth >= 6 ? deep_strips(nx, depth) : (depth == 5 ? step5_strips(nx) : (nx + STRIP_W - 1) / STRIP_W);
}

// What a row of a wall-column strip costs, in rows of an interior strip, in a pipe or a cavity (the scans: plan_march).  The
// velocity-inlet family has values of its own in plan_march (2.3 / 1.6) and none in band_extra, which no slab of that family ever
// reaches (lb_create): the two sites differ there, and band thickness is speed -- left as measured.
static double wall_strip_cost(int depth) { return depth >= 6 ? 2.1 : 1.2; }

MarchPlan plan_march(const PlanInputs *s, int rows, int depth, const MarchBands &bands, int reserve)
{
    MarchPlan m;
    const int strips = m.strips = march_strips(s->p.nx, depth);
    m.edge_seg_rows = 0;
    int segs, seg_rows, extra_items = 0;
    if (bands.count > 0) {
        segs = bands.count;
        seg_rows = bands.rows;
        m.seg_stride = bands.stride;
    } else {
        // as many wave-items as the chip holds at once (waves per CU from the kernel's register
        // budget), each marching an equal share of the rows
        // (lb_autotune's waves per CU belong to the depth it found fastest: the shallower launches of a run's remainder keep 8;
        //  k_deep: one wave per SIMD -- 512 registers, 36 KB of LDS per wave)
        const int waves_per_cu = depth >= 6 ? 4 : ((s->tuned_wpc > 0 && depth == s->tuned_steps) ? s->tuned_wpc : 8);
        // (k_step4: an item is a PAIR of segments, marched by the two waves of a workgroup from its middle line: two
        //  wave slots each; `capacity`, `segs`, `seg_rows` then count pairs)
        const int per_item = (depth >= 4) ? STEP4_WAVES : 1;
        const int capacity = (s->cu_count * waves_per_cu - reserve) / per_item;
        segs = capacity / strips;
        if (segs < 1) segs = 1;
        seg_rows = (rows + segs - 1) / segs;
        // (floor: grids of 1024^2 .. 2048^2 are latency-bound, not bandwidth-bound -- filling every wave slot
        //  with a short segment beats fewer, longer ones although each segment recomputes (d-1) [k_step4] or 2(d-1) rows:
        //  with the earlier floor of 16 rows 2048^2 ran at 142 k MLUPS, with 4..8 at 170 k: profiles/r01_sweep_variants.txt)
        if (seg_rows < 4 * per_item) seg_rows = 4 * per_item;
        segs = (rows + seg_rows - 1) / seg_rows;
        m.seg_stride = seg_rows;
        // k_step4 in a box with walls at its left and right end: the two wall-column strips get shorter segments (their
        // rows cost edge_cost times an interior strip's: the boundary rule of one cell per row and stage -- measured per
        // wave, tools/wave_timeline.py: +18 % pipe, +10..16 % cavity; the velocity-inlet columns also read the stored u, v),
        // within the same number of wave slots: pipe / cavity +5..8 %, velocity inlet +19..30 % (profiles/r02_experiments.txt)
        // (k_step5 has no halo-lane work, so the wall column's rule weighs more in its rows: velocity inlet, 8192^2, edge cost 1.2:
        //  301-305 k MLUPS, 1.6: 306-310 k, 2.0: 322-339 k, 2.5: 329-348 k, 3.0: 321-328 k; 4096^2: 252 / 274 / 290 / 298 / 276 k;
        //  pipe and cavity stay at 1.2: profiles/r04_experiments.txt section 10)
        // (k_deep, one wave per SIMD, the rule out of line: a wall-column strip's rows cost ~1.8 x an interior strip's -- per-wave
        //  timelines, profiles/r05_wave_timeline_walls.txt; scan 1.2 ... 3.0, k MLUPS, k_deep<7>: pipe 8192^2 392 (1.2-1.8) / 379
        //  (2.0-3.0), 4096^2 285 (1.2-1.5) / 322-325 (1.8-2.0) / 319-321 (2.2-3.0), 6144^2 372-377 (1.8-2.2) / 358 (3.0); cavity
        //  8192^2 395 (<= 1.8) / 370 (>= 2.0), 4096^2 303 / 318-321: profiles/r05_edge_cost_scan.txt.  Scanned again once the interior
        //  strips had got faster -- the hand-waited gather does nothing for a wall-column strip, whose out-of-line rule drains the
        //  memory counter at every call --: 1.8 | 2.0 | 2.2 | 2.5 | 3.2, k MLUPS, k_deep<7>: pipe 8192^2 394 | 419 | 420 | 416 | 420, 6144^2
        //  410 | 413 | 419 | 402 | 388, 4096^2 333 | 351 | 347 | 349 | 325; cavity 4096^2 346 | 351 | 353 | 350 | 328; config 5's image 4096^2
        //  310 | 320 | 320 | 309 | 289; k_deep<6> pipe 8192^2 381 | 406 | 403 | 406 | 407: profiles/r05_edge_cost_scan2.txt -> 2.1)
        const double edge_cost = s->p.bc_mode == LB_BC_VELOCITY_INLET ? (depth == 5 ? 2.3 : 1.6) : wall_strip_cost(depth);
        if (depth >= 4 && s->p.bc_mode != LB_BC_PERIODIC && strips >= 4 && edge_cost > 1.0 && segs * strips >= capacity / 2) {
            // the split of the wave slots between interior strips (segs_i pairs each) and the two wall-column strips (segs_e each) that
            // finishes first: min over segs_i of max(rows_i, edge_cost x rows_e).  (Until round 5: segs_i = capacity / (strips - 2 +
            // 2 edge_cost) rounded down, the remainder to the wall strips -- with few slots per strip the rounding gave them three
            // times the interior's pairs.)
            int best_i = 0, best_e = 0;
            double best_t = 1e30;
            // (from two below the closed form capacity / (strips - 2 + 2 edge_cost): a window of capacity / strips - 2 ... + 1 missed the
            //  optimum wherever the edge cost is high and the strips few -- the velocity-inlet family at 4096^2, cost 2.3, 18 strips:
            //  54 pairs per interior strip where 48 finish first; 269-272 k MLUPS against round 4's 286-297 k on the same box,
            //  profiles/r05_vs_r04_one_box.txt)
            const int si_lo = std::max(1, (int)(capacity / (strips - 2 + 2.0 * edge_cost)) - 2);
            for (int si = std::min(si_lo, std::max(1, capacity / strips - 2)); si <= capacity / strips + 1; ++si) {
                const int se = (capacity - (strips - 2) * si) / 2;
                if (se < si) continue;
                const int ri = (rows + si - 1) / si, re = (rows + se - 1) / se;
                if (re < 8 * per_item) continue;
                const double t = std::max((double)ri + (depth - 1), edge_cost * (re + (depth - 1)));
                if (t < best_t) { best_t = t; best_i = si; best_e = se; }
            }
            const int segs_i = best_i, segs_e = best_e;
            if (segs_i >= 1 && segs_e > segs_i) {
                const int rows_i = (rows + segs_i - 1) / segs_i, rows_e = (rows + segs_e - 1) / segs_e;
                seg_rows = rows_i;
                segs = (rows + rows_i - 1) / rows_i;
                m.seg_stride = rows_i;
                m.edge_seg_rows = rows_e;
                extra_items = 2 * ((rows + rows_e - 1) / rows_e - segs);
                if (extra_items < 0) extra_items = 0, m.edge_seg_rows = 0;
            }
        }
    }
    m.segs = segs;
    m.seg_rows = seg_rows;
    m.items = strips * segs + extra_items;
    return m;
}

// which of k_tile4's three shapes (launchers.h: lbk_launch_tile4)
int tile_shape_of(const PlanInputs *s)
{
    // 32 x 16 tiles (512 threads, two cells per thread, 49-60 VGPR: four workgroups per CU -- with 32 x 32 tiles and
    // four cells per thread the same kernel ran at 117 instead of 144 k MLUPS at 1024^2: occupancy is what hides
    // the LDS round trips); 16 x 16 tiles, one cell per thread, for grids that would not give every CU a workgroup
    // (round 1: two cells per thread from 900^2: 145 against 134 k at 1024^2; one below: 90 against 83 k at 512^2)
    const long long cells = (long long)s->p.nx * s->H;
    // (with one band of tile rows per XCD, two cells per thread: 32 x 32 tiles 150 k, 64 x 16 154-158 k against 175 k at 1024^2
    //  periodic, and further behind on larger grids: profiles/r03_experiments.txt section 15)
    // (two cells per thread from 576^2 -- 900^2 until the rings were stepped by whole waves: one / two cells per thread, MLUPS,
    //  periodic 512^2 122-124 / 123 k, 640^2 125-128 / 133-135 k, 768^2 145 / 156 k, 896^2 152 / 170 k; cavity 512^2 110 / 107 k,
    //  640^2 112 / 121 k, 896^2 139 / 156 k: profiles/r03_experiments.txt section 16)
    if (cells >= 576LL * 576) return 0;
    return cells >= 330LL * 330 ? 1 : 2;
}

// (launch-bound: single steps are replayed from a hipGraph, launch.cpp)
bool small_grid(const PlanInputs *s) { return (double)s->p.nx * s->H <= 768.0 * 768.0; }

// How many time steps the next launch of a run with `left` steps to go advances.  `allowed`: bit d set = the d-step kernel may be
// used (bit 1 always is).  A launch of a marching kernel costs about the same whatever number of steps it fuses (it moves the
// same bytes); `cost[d]` = what a d-step launch costs on this handle, in any one unit (launch_costs).  The cheapest way to split
// `left` into allowed depths, by dynamic programming over the last 64 steps of a run (before that: the deepest kernel); shallow
// launches first.  With the seed costs: 20 steps with depths up to 7 = 6 + 7 + 7, up to 6 = 4 + 4 + 6 + 6, up to 5 = 4 x 5.
int next_advance(int allowed, int left, const float *cost)
{
    int D = 1;
    for (int d = 2; d <= MAX_DEPTH; ++d)
        if (allowed & (1 << d)) D = d;
    if (left > 64) return D;
    float best[65];
    int first[65];                       // the shallowest launch of a cheapest split of m steps
    best[0] = 0.f; first[0] = 0;
    for (int m = 1; m <= left; ++m) {
        best[m] = 1e30f; first[m] = 1;
        for (int d = 1; d <= D && d <= m; ++d) {
            if (d > 1 && !(allowed & (1 << d))) continue;
            const float c = cost[d] + best[m - d];
            // (ties: the split whose shallowest launch is deepest -- fewer kinds of kernels in a run)
            const int f = (m - d) ? std::min(d, first[m - d]) : d;
            if (c < best[m] - 1e-6f || (c < best[m] + 1e-6f && f > first[m])) { best[m] = c; first[m] = f; }
        }
    }
    return first[left];
}
// Cost of a d-step launch on this handle, d = 1..MAX_DEPTH: what lb_autotune measured on it (milliseconds per launch, live
// steps), and for the depths it did not time the seeds -- one MI355X, 8192^2 periodic: k_step 0.79 ms, k_step2 0.85, k_step3 0.89,
// k_step4 0.86, k_step5 0.96, k_deep<6> 1.00, k_deep<7> 1.08 -- scaled to the measured ones.  (Until round 5 the seeds were the
// whole table, for every size and family.)
void launch_costs(const PlanInputs *s, float (&cost)[MAX_DEPTH + 1])
{
    static const float seed[MAX_DEPTH + 1] = {0.f, 0.79f, 0.85f, 0.89f, 0.86f, 0.96f, 1.00f, 1.08f};
    double num = 0., den = 0.;
    for (int d = 1; d <= MAX_DEPTH; ++d)
        if (s && s->depth_cost[d] > 0.f) { num += s->depth_cost[d]; den += seed[d]; }
    const float scale = den > 0. ? (float)(num / den) : 1.f;
    cost[0] = 0.f;
    for (int d = 1; d <= MAX_DEPTH; ++d) cost[d] = (s && s->depth_cost[d] > 0.f) ? s->depth_cost[d] : seed[d] * scale;
}
int next_advance(const PlanInputs *s, int allowed, int left)
{
    float cost[MAX_DEPTH + 1];
    launch_costs(s, cost);
    return next_advance(allowed, left, cost);
}
int depth_mask(bool two, bool three, bool four, bool five, bool six, bool seven)
{
    return 2 | (two ? 4 : 0) | (three ? 8 : 0) | (four ? 16 : 0) | (five ? 32 : 0) | (six ? 64 : 0) | (seven ? 128 : 0);
}

// slabs launch by launch (outside the halo cycle, or where none applies): one, two or three steps per launch
int slab_step_depths(const PlanInputs *s, int h)
{
    const int v = effective_variant(s);
    return depth_mask((v & LB_VAR_STEP2) && step2_applicable(s, h), (v & LB_VAR_STEP3) && step3_applicable(s, h));
}

// The halo cycle of a slab (slab.cpp): two D-step launches per halo exchange, ghost zone 2D rows deep.
// depth of the fused kernel the halo cycle of a slab runs on: 4 (eight-step cycle), 3 (six-step cycle) or 0
// (no cycle: exchange after every launch).  h = the smallest slab height of the run.
int cycle_depth(const PlanInputs *s, int h)
{
    const int v = effective_variant(s);
    if (!(v & LB_VAR_STEP3) || (v & LB_VAR_NO_CYCLE) || !step3_applicable(s, h) || h < 32) return 0;
    // (lb_set_slab_cycle: the caller's choice -- the ranks of a run time the candidates together and agree, bench.py / slabs.py --
    //  wherever that depth can run; elsewhere the automatic one)
    if (s->forced_cycle >= 3 && s->forced_cycle <= MAX_DEPTH && h >= 16 * s->forced_cycle &&
        !(s->forced_cycle >= 6 && s->p.bc_mode == LB_BC_VELOCITY_INLET))
        return s->forced_cycle;
    // (k_deep on slabs, round 5: the fourteen- / twelve-step cycle, ghost zone as deep)
    if ((v & LB_VAR_STEP7) && (v & LB_VAR_STEP6) && (v & LB_VAR_STEP5) && (v & LB_VAR_STEP4) && h >= 112) return 7;
    if ((v & LB_VAR_STEP6) && (v & LB_VAR_STEP5) && (v & LB_VAR_STEP4) && h >= 96) return 6;
    // (k_step5 on slabs: the ten-step cycle, ghost zone ten rows deep)
    if ((v & LB_VAR_STEP5) && (v & LB_VAR_STEP4) && h >= 80) return 5;
    return ((v & LB_VAR_STEP4) && h >= 64) ? 4 : 3;
}

// Thick edge bands (round 6).  The rows an edge band MUST cover are the 2D next to a slab edge (the halo is cut from them, D ghost rows
// are recomputed on the way); as 14-row marches behind six filling iterations they kept 2 x strips workgroup slots busy for a
// quarter of the launch and idle for the rest, while the interior's waves marched the longer for it (8192 x 1024 rows, one of eight
// slabs: 48 iterations per wave where 44 do; profiles/r05_slab_proxy_final.txt).  Nothing in the cycle's data flow fixes where the
// band ends: with bands B rows thicker -- E1: [-D, D+B), C1: [D+B, H-D-B); E2: [0, 2D+B), C2: [2D+B, H-2D-B) -- E1 still reads
// exactly what E2 and the exchange wrote, C2 only what C1 wrote, E2 waits for C1 and the next C1 for E2, as before.  B is chosen so
// that a band wave's march (x the wall-column strips' cost in a walled box) ends `slack` iterations before an interior wave's.
// Rank-local: the neighbours need not agree.
//
// Split bands (the default in lb_run).  With thick bands the exchange -- on the edge stream between E2 and the next E1 -- had only that
// head start to complete in: enough for the peer transport's one push kernel (one box, k MLUPS per GPU, bands of round 5 | thick:
// 8192 x 1024 rows 378 | 393, x 2048 419 | 453, x 4096 442 | 476 = the plain grid's rate), not for RCCL's pack, send / receive and unpack
// (371 | 315, 416 | 372, 442 | 339: profiles/r06_slab_proxy_bands.txt).  But only the OUTER 2D rows of a band have to do with the exchange:
//   E2a  rows [0, 2D)        the rows the halo is cut from        -> ev_edge -> the exchange, on the communication stream
//   E2b  rows [2D, 2D+B)     meanwhile, on the edge stream
//   E1b  rows [D, D+B)       of the next cycle: reads rows [0, 2D+B) only, no ghost row -- does not wait for the exchange
//   E1a  rows [-D, D)        the one launch that reads the ghost rows: waits for ev_halo
// so the exchange has from the end of E2a to the start of E1a, more than a whole launch, and every workgroup slot stays busy.
// (lb_run_group keeps each band one launch.)
// (Which transport.  RCCL's pack, send / receive, unpack take 30-160 us and never fitted a thick band's head start: one launch per band
//  331-341 | 356-357 | 363-380 k MLUPS per GPU at 8 | 4 | 2 slabs of a strong-scaled 8192^2, split 353-388 | 372-386 | 420-445
//  (profiles/r06_slab_proxy_split.txt).  The peer transport's exchange is one push kernel, ~16 us, and on that box one launch per band
//  did as well or 3 % better (370-386 | 437-443 | 461-468 against 372-383 | 424-426 | 460) -- but on two later boxes it lost 8-15 %
//  wherever the bands are long: three alternating repetitions, 8 | 4 | 2 | 1 slabs, one launch 398-403 | 384-408 | 417-436 | 432-456,
//  split 397-399 | 449-453 | 470-474 | 484 = 0.92 | 0.97 | 0.98 | 0.99 of the plain grids of those sizes
//  (profiles/r06_slab_proxy_peer_split_ab.txt; bench.py --force-slab-path: 415 k one launch, 467 k split).  With one launch per band
//  the next E1 queues behind E2 AND the exchange on one stream, and whether that chain keeps up with the interior depends on the box's
//  issue rate; split, nothing of a band but its outer 2D rows waits for anything.  Hence split for both transports.)
int band_extra(const PlanInputs *s, int D, bool split)
{
    if (D < 4) return 0;                                // (k_step2 / k_step3: one wave per strip and band, a few rows: as they were)
    // (one launch per band: the exchange must fit into the head start; split: only the launch gaps of the two parts do)
    const double slack = split ? 3.0 : 8.0;
    const int H = s->H;
    const int room = (H - 4 * D) / 2 - 8;               // the interior of the second launch keeps at least 16 rows
    if (room <= 0) return 0;
    const int strips = march_strips(s->p.nx, D);
    const int wpc = D >= 6 ? 4 : 8;
    const int segs = std::max(1, (s->cu_count * wpc - 2 * strips * STEP4_WAVES) / STEP4_WAVES / strips);    // interior pairs per strip
    const double cost = s->p.bc_mode == LB_BC_PERIODIC ? 1.0 : wall_strip_cost(D);
    int B = 0;
    for (int b = 2; b <= room; b += 2) {
        // a band wave's iterations: the band as one march of (2D + b) / 2 rows per wave, or -- split -- two marches, D and b / 2 rows
        const double band = cost * (split ? (D + (D - 1)) + (b / 2.0 + (D - 1)) : (2 * D + b) / 2.0 + (D - 1)) + slack;
        const double inner = (double)((H - 4 * D - 2 * b + segs - 1) / segs) / 2.0 + (D - 1);
        if (band > inner) break;
        B = b;
    }
    return B;
}

// Which fused depths a whole-grid handle may use: the variant bits (explicit or from the size heuristic), or --
// once lb_autotune has timed this grid -- everything applicable up to the depth it found fastest.
// Four steps per pass through LDS tiles (k_tile4) instead of the marching kernels: asked for (LB_VAR_TILES),
// found fastest by lb_autotune, or -- automatic -- on whole grids below ~1400^2 cells and on grids the marching
// kernels do not serve (27 k MLUPS at 256^2, 82 k at 512^2, 120 k at 1024^2, 138 k at 1280^2, against 19 / 57 /
// 113 / 129 k; from 1536^2 the marching kernel wins, 163 against 153 k: profiles/r01_sweep_variants.txt).
bool use_tile_kernel(const PlanInputs *s)
{
    if (!tile_applicable(s)) return false;
    if (s->variant >= 0) return (s->variant & LB_VAR_TILES) != 0;
    if (s->tuned_steps) return s->tuned_wpc < 0;
    // (walled boxes likewise: pipe 24 / 74 / 112 / 123 k at 256^2 / 512^2 / 1024^2 / 1280^2 against 16.5 / 55 / 95 / 113 k;
    //  marching from 1536^2: 136 against 130 k)
    // (round 3: the four-step marching kernel on segment pairs, against the tiles: periodic 1024^2 124 / 153 k MLUPS, 1280^2
    //  173 / 169 k, 1536^2 216 / 179 k, 2048^2 248 / 187 k; cavity 1024^2 99 / 148 k, 1280^2 146 / 166 k, 1536^2 180 / 176 k,
    //  2048^2 217 / 183 k: profiles/r03_experiments.txt; the change-over was at 1600^2, then 1250^2 / 1450^2)
    // (later in round 3: the tiles with one band of tile rows per XCD and the rings stepped by whole waves, marching / tiles:
    //  periodic 1792^2 220 / 235 k, 1920^2 229 / 239 k, 2048^2 243 / 207 k; cavity 1920^2 200 / 228 k, 2048^2 214 / 201 k; pipe
    //  1920^2 193 / 231 k, 2048^2 208 / 204 k, 2176^2 218 / 197 k: the tiles hold while the lattice pair fits the 256 MB
    //  Infinity Cache -- 1920^2 is 265 MB, 2048^2 302 MB -- in every family)
    // (round 4: five steps per pass on overlapping strips, k_step5 / tiles: periodic 1024^2 166 / 198 k, 1280^2 233 / 218 k, 1536^2
    //  261 / 240 k, 1792^2 294 / 249 k, 2048^2 305 / 209 k; cavity 1280^2 173 / 202 k, 1536^2 200 / 220 k, 1792^2 225 / 231 k,
    //  2048^2 259 / 194 k: profiles/r04_step5_sweep.txt; until then the change-over to k_step4 was at 1950^2)
    // (round 6, walled boxes, tiles | k_step5 | k_deep2<7>, k MLUPS, profiles/r06o_walled_tile_sweep.txt: pipe 1280^2 214 | 191 | 156, 1536^2
    //  230 | 227 | 221, 1664^2 236 | 248 | 252, 1792^2 238 | 253 | 280, 2048^2 207 | 263 | 302; cavity 1536^2 227 | 240 | 231, 1792^2 233 | 266 | 290;
    //  pipe + mask 1536^2 201 | 209 | 199, 1792^2 211 | 233 | 249: the walled change-over moves from 1850^2 to 1450^2)
    const double side = s->p.bc_mode == LB_BC_PERIODIC ? (s->has_mask ? 1200.0 : 1100.0) : 1450.0;
    return (double)s->p.nx * s->H < side * side || !step4_applicable(s);
}

int whole_grid_depths(const PlanInputs *s)
{
    if (use_tile_kernel(s)) return depth_mask(false, false, true);      // k_tile4 + single steps for the remainder
    if (s->variant < 0 && s->tuned_steps)
        return depth_mask(step2_applicable(s) && s->tuned_steps >= 2, step3_applicable(s) && s->tuned_steps >= 3,
                          step4_applicable(s) && s->tuned_steps >= 4, step5_applicable(s) && s->tuned_steps >= 5,
                          deep_applicable(s) && s->tuned_steps >= 6, deep_applicable(s) && s->tuned_steps >= 7);
    const int v = effective_variant(s);
    return depth_mask((v & LB_VAR_STEP2) && step2_applicable(s), (v & LB_VAR_STEP3) && step3_applicable(s), (v & LB_VAR_STEP4) && step4_applicable(s),
                      (v & LB_VAR_STEP5) && step5_applicable(s), (v & LB_VAR_STEP6) && deep_applicable(s), (v & LB_VAR_STEP7) && deep_applicable(s));
}

// the Cython path runs four steps per launch through LDS tiles (k1_tile4) unless the grid is too small for them or an
// explicit variant without LB_VAR_TILES asks for single steps (k1_fstep)
bool cython_tiles(const PlanInputs *s) { return s->p.nx >= 64 && s->H >= 64 && (s->variant < 0 || (s->variant & LB_VAR_TILES)); }

bool autotune_applies(const PlanInputs *s)
{
    return !s->multi_slab() && s->p.semantics != LB_SEM_CYTHON &&
           (step2_applicable(s) || step3_applicable(s) || tile_applicable(s));
}

// a remembered result of lb_autotune (tune.cpp: LB_TUNE_CACHE) names a kernel this handle can run
bool tune_entry_runs_here(const PlanInputs *s, int steps, int wpc)
{
    if (!autotune_applies(s) || steps < 1 || steps > MAX_DEPTH) return false;
    if (steps >= 6) return deep_applicable(s) && (wpc == 4 || (steps == 7 && wpc == 8));
    if (steps == 5) return step5_applicable(s) && (wpc == 8 || wpc == 6);
    if (steps == 4) return wpc < 0 ? tile_applicable(s) : (step4_applicable(s) && (wpc == 8 || wpc == 6 || wpc == 4));
    if (steps == 3) return step3_applicable(s) && (wpc == 8 || wpc == 6 || wpc == 4);
    if (steps == 2) return step2_applicable(s) && (wpc == 8 || wpc == 4);
    return wpc == 0;
}

// ---- behind the ABI's lb_plan_launches, lb_steps_per_launch, lb_hot_kernel --------------------------------------------------------
// Scalar lattices.  An explicit variant decides: its tile bit (LB_VAR_TILES) = k_ad_tile4 for every group of four steps, on any box
// (the kernel wraps or clips its regions itself); without the bit, k_ad_step.  Automatic (-1): by size, the rule below.
// The size rule (profiles/scalar_bench.txt: k_ad_step and the three tile shapes timed in alternation on one handle, both families, G = 0 and
// 0.01): the best tile shape ran 2.5-3.0 x k_ad_step's rate at 256^2 (launch-bound: 18-21 k MLUPS against 52-56 k), 2.1-2.3 x at 512^2,
// 2.0-2.5 x at 1024^2, 2.1-2.4 x at 2048^2, 2.2-2.6 x at 4096^2 and 2.3-2.75 x at 8192^2 (70 k against 162-192 k) -- faster in every case of
// every size measured, so the tiles are taken over exactly that range; smaller and larger boxes were not measured and stay on k_ad_step.
// The shape by size as for k_tile4 (tile_shape_of) is the sweep's best one at 256^2 (16 x 16), 512^2 (32 x 16, one cell per thread) and
// from 2048^2 (two per thread); at 1024^2 it is the periodic family's best and 5 % behind the other 32 x 16 shape in the OPEN family.
static const double SCALAR_TILE_MIN_CELLS = 256.0 * 256.0, SCALAR_TILE_MAX_CELLS = 8192.0 * 8192.0;
static const double SCALAR_NOISY_OPEN_TILE_END_CELLS = 1024.0 * 1024.0;     // (noisy handles of the OPEN family: tiles below, k_ad_step from here)
// Multicomponent Shan-Chen fluids: variant 0 = the two-launch step, 1 = the one-launch step.  The planner's choice (-1) is the
// one-launch step at every size: on one MI355X it is 1.00-1.21 x the two-launch step at 256^2 ... 8192^2 with one, two and three
// fluids, but for 0.97 x at 1024^2 with two (profiles/multifluid_bench.txt, tools/multifluid_bench.py) -- no size rule to draw from that.
bool multifluid_one_launch(const PlanInputs *s) { return s->variant != 0; }
// Surfactant-propelled colonies: the same two variants.  The planner's choice (-1) is the one-launch step at every size: on one MI355X
// it is 1.19-1.61 x the two-launch step at 256^2 ... 8192^2 in both modes (profiles/rocket_bench.txt, tools/rocket_bench.py).
bool rocket_one_launch(const PlanInputs *s) { return s->variant != 0; }
// A flow and the `count` scalars it carries (lb_run_advected): form 1, the one-launch step k_fa_step, or form 0, k_step<MACRO> and one
// k_ad_step per scalar.  The planner's choice (-1) is whichever tools/advected_bench.py measured faster at the size, per count
// (profiles/advected_bench.txt; DESIGN.md section 19 has the table).  On one MI355X that is form 1 at every size measured, 256^2 ...
// 8192^2, with one scalar and with two: 1.10-1.42 x form 0 with one scalar, 1.13-1.67 x with two (the byte ratio is 164 / 144 and
// 244 / 216; below 1024^2 a step is its launches), and 1.24-1.38 x today's sequence of existing calls from 2048^2 up.  The sizes and
// the count stay arguments: a box on which form 0 wins somewhere gets its threshold here.
int advected_form(long long cells, int count, int form)
{
    if (form >= 0) return form;
    (void)cells; (void)count;
    return 1;
}

bool scalar_use_tiles(const PlanInputs *s)
{
    if (s->multifield() || s->poisson() || s->porous() || s->multifluid() || s->rocket()) return false;      // (no tiles for coupled sets, the Poisson solver and the porous-medium fluid: k_mf_step / k_ps_step / k_pm_step, one step per launch)
    if (s->variant >= 0) return (s->variant & LB_VAR_TILES) != 0;
    const double cells = (double)s->p.nx * s->H;
    // The noisy collision (lb_set_noise; profiles/scalar_bench.txt, the noise column: 256^2 ... 8192^2, all six sizes, both families).
    // k_ad_step draws one Philox block per lane-of-four and keeps 0.97-1.00 x its noiseless rate from 1024^2 up; k_ad_tile4 with its noise
    // plane in LDS falls to 0.43-0.63 x its own.  Best noisy tile shape over the noisy k_ad_step, 256^2, 512^2, ... 8192^2:
    //   PERIODIC  2.15  1.57  1.33  1.58  1.57  1.62   faster at every size measured: the noiseless range stands
    //   OPEN      2.10  1.39  0.99  1.03  0.98  0.97   faster at 256^2 and 512^2; from 1024^2 up within the samples' spread of 1 (0.2-4.9 %),
    //                                                   not faster: k_ad_step
    if (s->noisy && s->p.bc_mode != LB_BC_PERIODIC && cells >= SCALAR_NOISY_OPEN_TILE_END_CELLS) return false;
    return cells >= SCALAR_TILE_MIN_CELLS && cells <= SCALAR_TILE_MAX_CELLS;
}

// With an explicit variant the bits that pick k_step's rows per workgroup (LB_VAR_ROWS: meaningless here) pick the tile shape:
// 0 = by size as for k_tile4, 1 / 2 / 3 = shape 0 / 1 / 2 (32 x 16 two cells per thread, 32 x 16 one, 16 x 16 one).
int scalar_tile_shape(const PlanInputs *s)
{
    if (s->variant >= 0 && (s->variant & LB_VAR_ROWS)) return ((s->variant & LB_VAR_ROWS) >> 2) - 1;
    return tile_shape_of(s);
}

int scalar_next_advance(const PlanInputs *s, int left)
{
    if (left <= 0) return 0;
    return (left >= TILE_T && scalar_use_tiles(s)) ? TILE_T : 1;
}

int plan_launches(const PlanInputs *s, int n_steps, int *depths, int max_launches)
{
    if (s->scalar() || s->porous() || s->multifluid()) {
        int n = 0;
        for (int left = n_steps; left > 0; ++n) {
            const int adv = scalar_next_advance(s, left);
            if (depths && n < max_launches) depths[n] = adv;
            left -= adv;
        }
        return n;
    }
    const int allowed = whole_grid_depths(s);
    int n = 0;
    for (int left = n_steps; left > 0; ++n) {
        const int adv = next_advance(s, allowed, left);
        if (depths && n < max_launches) depths[n] = adv;
        left -= adv;
    }
    return n;
}

int steps_per_launch(const PlanInputs *s)
{
    if (s->scalar() || s->porous() || s->multifluid()) return scalar_use_tiles(s) ? TILE_T : 1;
    if (s->p.semantics == LB_SEM_CYTHON) return cython_tiles(s) ? TILE_T : 1;
    const int h = s->agreed_h();
    if (s->multi_slab() && cycle_depth(s, h)) return cycle_depth(s, h);
    const int depths = s->multi_slab() ? slab_step_depths(s, h) : whole_grid_depths(s);
    int n = 1;
    for (int d = 2; d <= MAX_DEPTH; ++d)
        if (depths & (1 << d)) n = d;
    return n;
}

void hot_kernel(const PlanInputs *s, char *buf, int buflen)
{
    static const char *const bc_names[] = {"PIPE", "PERIODIC", "CAVITY", "VELOCITY_INLET", "PIPE, D2Q9i"};
    if (s->multifluid()) {
        if (multifluid_one_launch(s)) {
            snprintf(buf, (size_t)buflen, "k_mc_step (multicomponent Shan-Chen fluids: one launch per step -- pull-stream + densities of the owned rows and their halo into LDS, barrier, interaction forces + barycentric velocity + Guo-forced collide + reactions)<%s%s>",
                     s->p.bc_mode == LB_BC_PERIODIC ? "PERIODIC" : "ZERO_GRADIENT", s->has_field ? ", FIELD" : "");
            return;
        }
        snprintf(buf, (size_t)buflen, "k_mc_moments + k_mc_collide (multicomponent Shan-Chen fluids: two launches per step -- pull-stream + densities, then pull-stream + interaction forces + barycentric velocity + Guo-forced collide + reactions)<%s%s>",
                 s->p.bc_mode == LB_BC_PERIODIC ? "PERIODIC" : "ZERO_GRADIENT", s->has_field ? ", FIELD" : "");
        return;
    }
    if (s->rocket()) {
        if (rocket_one_launch(s))
            snprintf(buf, (size_t)buflen, "k_ry_step (surfactant-propelled colony: one launch per step -- pull-stream of both lattices + the two stencil operands of the %d owned rows and their halo into LDS, barrier, velocity and forces + linear-equilibrium collide)<PERIODIC>", RY_ROWS);
        else
            snprintf(buf, (size_t)buflen, "k_ry_moments + k_ry_collide (surfactant-propelled colony: two launches per step -- pull-stream + densities, then pull-stream + velocity and forces + linear-equilibrium collide)<PERIODIC>");
        return;
    }
    if (s->porous()) {
        snprintf(buf, (size_t)buflen, "k_pm_step (forced flow in a porous medium: one fused pull-stream + moments + drag and body force + Guo-forced collide pass)<%s%s>",
                 s->p.bc_mode == LB_BC_PERIODIC ? "PERIODIC" : "ZERO_GRADIENT", s->has_field ? ", FIELD" : "");
        return;
    }
    if (s->poisson()) {
        snprintf(buf, (size_t)buflen, "k_ps_step (LB Poisson solver: one fused pull-stream + prescribed-value walls + relaxation pass that also leaves the convergence sums)<DIRICHLET>");
        return;
    }
    if (s->multifield()) {
        snprintf(buf, (size_t)buflen, "k_mf_step (coupled scalar lattices: one fused pull-stream + linear-equilibrium collide pass for all fields)<%s>",
                 s->p.bc_mode == LB_BC_PERIODIC ? "PERIODIC" : "BOX");
        return;
    }
    if (s->scalar()) {
        snprintf(buf, (size_t)buflen, "%s<%s>",
                 scalar_use_tiles(s) ? "k_ad_tile4 (scalar lattice: four steps per launch in LDS tiles)"
                                     : "k_ad_step (scalar lattice: one fused pull-stream + linear-equilibrium collide pass)",
                 s->p.bc_mode == LB_BC_PERIODIC ? "PERIODIC" : "OPEN");
        return;
    }
    const char *kernel = "k_step";
    if (s->p.semantics == LB_SEM_CYTHON)
        kernel = cython_tiles(s) ? "k1_tile4 (Cython path, LDS tiles)" : "k1_fstep (Cython path)";
    else {
        const int spl = steps_per_launch(s);
        if (!s->multi_slab() && use_tile_kernel(s) && spl == 4) kernel = "k_tile4 (LDS tiles)";
        else if (spl == 7 && deep2_chosen(s)) kernel = "k_deep2<7> (marching strips, seven steps per pass, two waves per strip and direction -- stages 1-4 / 5-7 --, two waves per SIMD)";
        else if (spl == 7) kernel = "k_deep<7> (marching strips, seven steps per pass, one wave per SIMD, stage windows in registers + LDS, gather one row ahead)";
        else if (spl == 6) kernel = "k_deep<6> (marching strips, six steps per pass, one wave per SIMD, stage windows in registers + LDS, gather one row ahead)";
        else if (spl == 5) kernel = "k_step5 (marching strips, five steps per pass: two stage windows in registers, two in wave-private LDS)";
        else if (spl == 4) kernel = "k_step4 (marching strips, stage windows in registers + wave-private LDS)";
        else if (spl == 3) kernel = "k_step3 (marching strips, register windows)";
        else if (spl == 2) kernel = "k_step2 (marching strips, register window)";
        else kernel = "k_step (one fused pull-stream + collide pass)";
    }
    const int n = snprintf(buf, (size_t)buflen, "%s<%s%s>", kernel, bc_names[kernel_bc(s)], s->has_mask ? ", MASK" : "");
    if (s->tuned_steps && s->tuned_wpc > 0 && s->tuned_steps < 6 && strncmp(kernel, "k_step", 6) == 0 && kernel[6] != ' ' && n > 0 && n < buflen)
        snprintf(buf + n, (size_t)(buflen - n), ", tuned: %d waves per CU", s->tuned_wpc);
}
