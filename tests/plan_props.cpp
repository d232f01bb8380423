// plan_props.cpp -- the launch planner's invariants, swept on a host.  A stand-alone program: its own main, plan.h, linked with
// plan.cpp and nothing else (tests/test_plan_cpu.py builds and runs it, once plain and once under the address and undefined-
// behaviour sanitizers).  One line per property, "name cases=N bad=M", then the first few offenders; exit status 1 if any bad > 0.
//
//   plan_props                           the whole sweep
//   plan_props --thin                    a thinner sweep of the same properties (the sanitizer build)
//   plan_props --classify nx ny bc d     the geometry class of the d-step marching launch of a whole nx x ny grid of family bc
//                                        (0 pipe, 1 periodic, 2 cavity, 3 velocity inlet) on 256 CUs: tests/march_shapes.py
//   plan_props --onset nx bc d           the smallest heights at which that launch splits its wall strips (how the table was drawn up)
//
// The properties are the comments of plan.h / plan.cpp read as checks; the numbering (P1 ... P8) is the one in the docstring of
// tests/test_plan_cpu.py, which also records what each of seven planted defects turns red.
#include "plan.h"

#include <algorithm>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <array>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

// ---- bookkeeping -----------------------------------------------------------------------------------------------------------------
struct Prop {
    const char *name;
    long long cases = 0, bad = 0;
    std::vector<std::string> first;
    explicit Prop(const char *n) : name(n) {}
    void fail(const std::string &what)
    {
        ++bad;
        if (first.size() < 5) first.push_back(what);
    }
    int report() const
    {
        printf("%s cases=%lld bad=%lld\n", name, cases, bad);
        for (const std::string &f : first) printf("    %s\n", f.c_str());
        return bad ? 1 : 0;
    }
};

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// a small generator of its own: the same cases on every host
struct Rng {
    unsigned long long s;
    explicit Rng(unsigned long long seed) : s(seed * 2862933555777941757ULL + 3037000493ULL) {}
    unsigned next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(s >> 33); }
    int below(int n) { return (int)(next() % (unsigned)n); }
};

// ---- inputs ----------------------------------------------------------------------------------------------------------------------
// a handle's plain data as lb_create fills it in (lb_hip.cpp): H rows of a box of nx x ny cells
PlanInputs inputs(int nx, int ny, int H, int bc, int cu = 256, int semantics = LB_SEM_OPENCL, int flags = 0)
{
    PlanInputs s;
    s.p = lb_params();
    s.p.nx = nx; s.p.ny = ny; s.p.local_ny = H; s.p.y0 = 0; s.p.omega = 1.f;
    s.p.semantics = semantics; s.p.bc_mode = bc; s.p.flags = flags;
    s.H = H;
    s.pitch = ((long long)nx + 63) / 64 * 64;
    if (flags & LB_FLAG_PLANAR) { s.rowp = s.pitch; s.plane = (long long)(H + 2 * GHOST) * s.pitch; }
    else { s.rowp = 9 * s.pitch; s.plane = s.pitch; }
    s.lat_floats = 9 * (long long)(H + 2 * GHOST) * s.pitch;
    s.cu_count = cu;
    return s;
}

// launch_march (launch.cpp) has a kernel of this depth for this boundary family
bool family_has_kernel(int depth, int bc) { return depth >= 1 && depth <= MAX_DEPTH && !(depth >= 6 && bc == LB_BC_VELOCITY_INLET); }

// ---- the kernels' item decode, restated ONCE -------------------------------------------------------------------------------------
// It mirrors, line for line, the prologues of
//   k_step2, k_step3   kernels_fused.h   (four items per workgroup, grid (items + 3) / 4; no wall-strip items)
//   k_step4            kernels_step4.h
//   k_step5            kernels_step5.h
//   k_deep<6>, <7>     kernels_deep.h
//   k_deep2<7>         kernels_deep2.h
// and launch_march / launch_marching (launch.cpp), which hand MarchPlan to them as strips, nsegs, seg_rows, seg_stride,
// edge_seg_rows, row_begin, row_end.  The GPU table (tests/march_shapes.py, test_gpu_march_geometry.py) ties this restatement to
// the kernels themselves.
int xcd_item(int wg, int nwg)
{
    const int blk = wg & ~63, i = wg & 63;
    return (blk + 64 <= nwg) ? blk + (i & 7) * 8 + (i >> 3) : wg;
}

struct Launch {
    int depth, row_begin, row_end;
    MarchPlan m;
    int workgroups() const { return depth >= 4 ? m.items : (m.items + 3) / 4; }
    int waves() const { return depth >= 4 ? 1 : 4; }         // decodes per workgroup (from k_step4 on the waves of a workgroup share one)
};

// what one decode comes to: false = the kernel returns without marching
struct Item { int item, sx, sy, ya, yb, ym; };
bool decode(const Launch &L, int wg, int w, Item &it)
{
    const MarchPlan &m = L.m;
    const int strips = m.strips, nsegs = m.segs;
    int seg_rows = m.seg_rows, stride = m.seg_stride;
    if (L.depth < 4) {
        const int item = it.item = xcd_item(wg, L.workgroups()) * 4 + w;
        it.sx = item % strips; it.sy = item / strips;
        if (it.sy >= nsegs) return false;
    } else {
        const int item = it.item = xcd_item(wg, L.workgroups());
        if (item < strips * nsegs) {
            it.sx = item % strips;
            it.sy = item / strips;
        } else {
            if (!m.edge_seg_rows) return false;
            const int j = item - strips * nsegs;
            it.sx = (j & 1) ? strips - 1 : 0;
            it.sy = nsegs + (j >> 1);
        }
        if (m.edge_seg_rows && (it.sx == 0 || it.sx == strips - 1)) stride = seg_rows = m.edge_seg_rows;
    }
    it.ya = L.row_begin + it.sy * stride;
    if (it.ya >= L.row_end) return false;
    it.yb = std::min(it.ya + seg_rows, L.row_end);
    it.ym = it.ya + (it.yb - it.ya) / 2;
    return true;
}

// ---- P1: every output row of every strip exactly once ------------------------------------------------------------------------------
struct Range { int lo, hi; };

// The row intervals of the marching items of one launch, per strip and in the order of their segment index (= ascending rows: the
// stride is positive), must tile `want` -- one range, or a band launch's two -- exactly once.  Scratch is kept between calls.
// (Whether a launch covers its rows is a function of what the kernel is handed, so a launch that was found right once -- for another
//  family, CU count or tuning word that led to the same numbers -- is not decoded again: most of the sweep's speed.)
struct Coverage {
    typedef std::array<int, 14> Key;
    struct KeyHash {
        size_t operator()(const Key &k) const
        {
            unsigned long long h = 1469598103934665603ULL;
            for (int v : k) h = (h ^ (unsigned)v) * 1099511628211ULL;
            return (size_t)(h ^ (h >> 29));
        }
    };
    std::unordered_set<Key, KeyHash> right;
    std::vector<int> ya, yb;            // [sx * slots + sy]; ya == INT_MIN: no item
    bool check(const Launch &L, const Range *want, int nwant, bool balanced, std::string &why)
    {
        const MarchPlan &m = L.m;
        const Key key = {L.depth, L.row_begin, L.row_end, m.strips, m.segs, m.seg_rows, m.seg_stride, m.edge_seg_rows, m.items,
                         nwant, want[0].lo, want[0].hi, want[nwant - 1].lo, balanced ? 1 : 0};
        if (right.count(key)) return true;
        if (!decode_all(L, want, nwant, balanced, why)) return false;
        right.insert(key);
        return true;
    }
    bool decode_all(const Launch &L, const Range *want, int nwant, bool balanced, std::string &why)
    {
        const MarchPlan &m = L.m;
        if (m.strips < 1 || m.segs < 1 || m.seg_rows < 1 || m.items < 1 || m.seg_stride < 1 || m.edge_seg_rows < 0) { why = "segs, seg_rows, items or stride below 1"; return false; }
        if (L.depth < 4 && (m.edge_seg_rows || m.items != m.strips * m.segs)) { why = "wall-strip items in a launch of k_step2 / k_step3, which decode none"; return false; }
        if (m.items < m.strips * m.segs || ((m.items - m.strips * m.segs) & 1)) { why = "items below strips x segs, or an odd number of extra ones"; return false; }
        const int slots = m.segs + (m.items - m.strips * m.segs) / 2;
        ya.assign((size_t)m.strips * slots, INT_MIN);
        yb.assign((size_t)m.strips * slots, INT_MIN);
        const int nwg = L.workgroups(), waves = L.waves();
        for (int wg = 0; wg < nwg; ++wg)
            for (int w = 0; w < waves; ++w) {
                Item it;
                const bool runs = decode(L, wg, w, it);
                if (balanced && it.item < m.strips * m.segs && (!runs || it.yb <= it.ya)) { why = "an empty item below strips x segs"; return false; }
                if (!runs) continue;
                if (it.sx < 0 || it.sx >= m.strips || it.sy < 0 || it.sy >= slots) { why = "an item outside the strips or segments"; return false; }
                const size_t k = (size_t)it.sx * slots + it.sy;
                if (ya[k] != INT_MIN) { why = "a segment marched by two items"; return false; }
                if (it.yb <= it.ya || it.ym < it.ya || it.ym > it.yb) { why = "an empty interval"; return false; }
                ya[k] = it.ya; yb[k] = it.yb;
            }
        for (int sx = 0; sx < m.strips; ++sx) {
            int r = 0, at = want[0].lo;                 // the range being filled, and how far
            for (int sy = 0; sy < slots; ++sy) {
                const size_t k = (size_t)sx * slots + sy;
                if (ya[k] == INT_MIN) continue;
                if (r < nwant && at == want[r].hi && ++r < nwant) at = want[r].lo;
                if (r >= nwant || ya[k] != at || yb[k] > want[r].hi) {
                    why = fmt("strip %d: rows [%d, %d) where row %d was due", sx, ya[k], yb[k], r < nwant ? at : -1);
                    return false;
                }
                at = yb[k];
            }
            if (r != nwant - 1 || at != want[r].hi) { why = fmt("strip %d: rows from %d on are never marched", sx, at); return false; }
        }
        return true;
    }
};

// ---- the sweep's axes ------------------------------------------------------------------------------------------------------------
bool THIN = false;
const int CUS[4] = {256, 304, 64, 8};
const int FAMILIES[4] = {LB_BC_PIPE, LB_BC_PERIODIC, LB_BC_CAVITY, LB_BC_VELOCITY_INLET};
const int WPCS[4] = {0, 4, 6, 8};

// widths from 512: every one up to 1500, thinner above, up to 9000 (periodic boxes: multiples of four only, step3_applicable)
std::vector<int> widths()
{
    std::vector<int> w;
    for (int nx = 512; nx <= 1500; ++nx) w.push_back(nx);
    for (int nx = 1504; nx <= 9000; nx += (nx < 3000 ? 244 : 748)) w.push_back(nx);
    w.push_back(9000);
    return w;
}
// launch rows: every value from 1 to 300, thinner up to 8192
std::vector<int> heights()
{
    std::vector<int> h;
    for (int r = 1; r <= 300; r += THIN ? 3 : 1) h.push_back(r);
    for (int r = 301; r <= 8192; r += (THIN ? 5 : 1) * (r < 1200 ? 29 : (r < 4200 ? 97 : 389))) h.push_back(r);
    for (int r : {1546, 1553, 3091, 3105, 3856, 3857, 8191, 8192}) h.push_back(r);
    return h;
}

// ---- P1 + P2 on balanced launches ------------------------------------------------------------------------------------------------
// plan_march reads the width through march_strips alone: the whole check runs on the first width of every strip count, and every
// other width is held to giving the plan of that first one (so a planner that starts to read nx elsewhere is seen).
void sweep_balanced(Prop &p1, Prop &p2, Prop &p1w)
{
    Coverage cov;
    const std::vector<int> W = widths(), R = heights();
    for (int cu : CUS)
        for (int bc : FAMILIES)
            for (int depth = 2; depth <= MAX_DEPTH; ++depth) {
                if (!family_has_kernel(depth, bc)) continue;
                for (int wpc : WPCS) {
                    int seen_strips = 0, first_nx = 0;
                    for (int nx : W) {
                        if (bc == LB_BC_PERIODIC && nx % 4) continue;
                        PlanInputs s = inputs(nx, 8192, 8192, bc, cu);
                        s.tuned_wpc = wpc; s.tuned_steps = wpc ? depth : 0;
                        const int strips = march_strips(nx, depth);
                        const bool first = strips != seen_strips;
                        if (first) { seen_strips = strips; first_nx = nx; }
                        PlanInputs s0 = s;
                        s0.p.nx = first_nx;
                        for (size_t ri = 0; ri < R.size(); ri += first ? 1 : 29) {
                            const int rows = R[ri];
                            const int reserves[2] = {0, 2 * strips * (depth >= 4 ? STEP4_WAVES : 1)};     // launch_interior's (slab.cpp)
                            for (int reserve : reserves) {
                                const MarchPlan m = plan_march(&s, rows, depth, MarchBands{}, reserve);
                                if (!first) {
                                    if (reserve) continue;
                                    ++p1w.cases;
                                    const MarchPlan m0 = plan_march(&s0, rows, depth, MarchBands{}, reserve);
                                    if (memcmp(&m, &m0, sizeof(m)))
                                        p1w.fail(fmt("nx %d and %d (both %d strips), %d rows, depth %d: different plans", nx, first_nx, strips, rows, depth));
                                    continue;
                                }
                                const int row_begin = (rows * 7 + depth) % 23 - 7;            // (a slab's E1 starts below row 0)
                                const Launch L = {depth, row_begin, row_begin + rows, m};
                                const Range want = {row_begin, row_begin + rows};
                                std::string why;
                                ++p1.cases;
                                if (!cov.check(L, &want, 1, true, why))
                                    p1.fail(fmt("cu %d bc %d depth %d wpc %d nx %d rows %d reserve %d: %s [strips %d segs %d seg_rows %d edge %d items %d]",
                                                cu, bc, depth, wpc, nx, rows, reserve, why.c_str(), m.strips, m.segs, m.seg_rows, m.edge_seg_rows, m.items));
                                // P2: one round of the resident waves
                                const int waves_per_cu = depth >= 6 ? 4 : (wpc ? wpc : 8);       // (k_deep, k_deep2: 4 whatever lb_autotune's word, seven steps at "8" among them)
                                const int per_item = depth >= 4 ? STEP4_WAVES : 1;
                                const int capacity = (cu * waves_per_cu - reserve) / per_item;
                                ++p2.cases;
                                const int segs_e = m.segs + (m.items - m.strips * m.segs) / 2;
                                if (m.items > std::max(capacity, m.strips))
                                    p2.fail(fmt("cu %d bc %d depth %d wpc %d nx %d rows %d reserve %d: %d items, %d slots", cu, bc, depth, wpc, nx, rows, reserve, m.items, capacity));
                                // (a wall split: the wall strips' segments are shorter than the interior's.  Where the two slot counts the planner
                                //  chose round to the same rows -- 245 and 246 pairs of 3916 rows: 16 each -- edge_seg_rows == seg_rows says what no split says)
                                else if (m.edge_seg_rows && (m.edge_seg_rows > m.seg_rows || segs_e < m.segs || (m.edge_seg_rows < m.seg_rows && segs_e <= m.segs) ||
                                                             m.edge_seg_rows < 8 * per_item || bc == LB_BC_PERIODIC || depth < 4))
                                    p2.fail(fmt("cu %d bc %d depth %d wpc %d nx %d rows %d reserve %d: wall split of %d against %d segments, %d rows each",
                                                cu, bc, depth, wpc, nx, rows, reserve, segs_e, m.segs, m.edge_seg_rows));
                            }
                        }
                    }
                }
            }
}

// ---- P1 on the launches of a slab: bands as launch_bands forms them, interiors as launch_interior does -----------------------------
struct SlabLaunches {
    Coverage &cov;
    Prop &p1;
    const PlanInputs *s;
    int D;
    // launch_bands (slab.cpp)
    void bands(int lo_s, int hi_s, int lo_n, int hi_n, const char *what)
    {
        if (hi_s - lo_s == hi_n - lo_n) {
            MarchBands b;
            b.count = 2; b.rows = hi_s - lo_s; b.stride = lo_n - lo_s;
            const Range want[2] = {{lo_s, hi_s}, {lo_n, hi_n}};
            one(lo_s, hi_n, b, 0, want, 2, what);
            return;
        }
        for (int i = 0; i < 2; ++i) {
            MarchBands b;
            b.count = 1; b.rows = i ? hi_n - lo_n : hi_s - lo_s;
            const Range want = {i ? lo_n : lo_s, i ? hi_n : hi_s};
            one(want.lo, want.hi, b, 0, &want, 1, what);
        }
    }
    // launch_interior (slab.cpp)
    void interior(int lo, int hi, const char *what)
    {
        const Range want = {lo, hi};
        one(lo, hi, MarchBands{}, 2 * march_strips(s->p.nx, D) * (D >= 4 ? STEP4_WAVES : 1), &want, 1, what);
    }
    void one(int row_begin, int row_end, const MarchBands &b, int reserve, const Range *want, int nwant, const char *what)
    {
        ++p1.cases;
        if (row_end <= row_begin) {         // launch_marching launches nothing: right only if nothing is wanted
            p1.fail(fmt("%s: nx %d H %d D %d: an empty launch", what, s->p.nx, s->H, D));
            return;
        }
        if (b.count > 0 && (b.rows < 1 || (b.count == 2 && b.stride < b.rows))) {
            p1.fail(fmt("%s: nx %d H %d D %d: bands of %d rows %d apart", what, s->p.nx, s->H, D, b.rows, b.stride));
            return;
        }
        MarchBands bb = b;
        if (bb.count == 1) bb.stride = 0;
        const MarchPlan m = plan_march(s, row_end - row_begin, D, bb, reserve);
        Launch L = {D, row_begin, row_end, m};
        if (b.count == 1) L.m.seg_stride = std::max(1, m.seg_stride);     // (one segment: the kernels never multiply by it)
        std::string why;
        if (!cov.check(L, want, nwant, b.count == 0, why))
            p1.fail(fmt("%s: cu %d bc %d nx %d H %d D %d rows [%d, %d): %s", what, s->cu_count, s->p.bc_mode, s->p.nx, s->H, D, row_begin, row_end, why.c_str()));
    }
};

void sweep_slabs(Prop &p1, Prop &p3)
{
    Coverage cov;
    const int nxs[] = {512, 724, 964, 1000, 1236, 2048, 3751, 4096, 8192};
    for (int cu : CUS)
        for (int bc : FAMILIES)
            for (int nx : nxs) {
                if (bc == LB_BC_VELOCITY_INLET) continue;         // (whole grids only: lb_create refuses a slab of that family)
                if (bc == LB_BC_PERIODIC && nx % 4) continue;
                std::vector<int> Hs;
                for (int H = 16; H <= 400; H += THIN ? 3 : 1) Hs.push_back(H);
                for (int H = 401; H <= 8192; H += (THIN ? 4 : 1) * (H < 1500 ? 13 : 211)) Hs.push_back(H);
                for (int H : Hs) {
                    PlanInputs s = inputs(nx, 4 * H, H, bc, cu, LB_SEM_OPENCL, LB_FLAG_HALO);
                    for (int D = 2; D <= MAX_DEPTH; ++D) {
                        // P3 (band_extra reads neither the family's kernels nor the height's lower bound: every H, every D)
                        int Bs[2];
                        for (int split = 0; split < 2; ++split) {
                            const int B = Bs[split] = band_extra(&s, D, split != 0);
                            ++p3.cases;
                            if (B < 0 || (B & 1) || (D < 4 && B) || (B > 0 && (H - 4 * D - 2 * B < 16 || 2 * D + B > H - 2 * D - B)))
                                p3.fail(fmt("cu %d bc %d nx %d H %d D %d split %d: B = %d", cu, bc, nx, H, D, split, B));
                        }
                        if (!family_has_kernel(D, bc)) continue;
                        SlabLaunches sl = {cov, p1, &s, D};
                        // slab_step_launch: two or three steps, three rows at each end
                        if (D <= 3 && H >= (D == 2 ? 16 : 32)) {
                            sl.bands(0, 3, H - 3, H, "slab_step_launch bands");
                            sl.interior(3, H - 3, "slab_step_launch interior");
                        }
                        // the halo cycle (cycle_depth: from 16 D rows where the caller fixes the depth, never below 32)
                        if (D < 3 || H < 16 * D || H < 32) continue;
                        for (int split = 0; split < 2; ++split) {
                            const int B = Bs[split];
                            if (B < 0 || 2 * D + B > H - 2 * D - B) continue;        // (P3 has it)
                            for (int ghosts = 0; ghosts < 4; ++ghosts) {               // a neighbour below / above or not; the last launch of a run has none
                                const int lo = (ghosts & 1) ? -D : 0, hi = (ghosts & 2) ? H + D : H;
                                if (split && B > 0) {
                                    sl.bands(D, D + B, H - D - B, H - D, "E1b");
                                    sl.bands(lo, D, H - D, hi, "E1a");
                                } else
                                    sl.bands(lo, D + B, H - D - B, hi, "E1");
                            }
                            sl.interior(D + B, H - D - B, "C1");
                            if (split && B > 0) {
                                sl.bands(0, 2 * D, H - 2 * D, H, "E2a");
                                sl.bands(2 * D, 2 * D + B, H - 2 * D - B, H - 2 * D, "E2b");
                            } else
                                sl.bands(0, 2 * D + B, H - 2 * D - B, H, "E2");
                            if (H - 2 * D - B > 2 * D + B) sl.interior(2 * D + B, H - 2 * D - B, "C2");
                        }
                    }
                }
            }
}

// ---- P4: plan_launches -----------------------------------------------------------------------------------------------------------
bool depth_allowed_here(const PlanInputs *s, int d)
{
    if (d == 1) return true;
    if (!(whole_grid_depths(s) & (1 << d))) return false;
    switch (d) {
    case 2: return step2_applicable(s);
    case 3: return step3_applicable(s);
    case 4: return use_tile_kernel(s) ? tile_applicable(s) : step4_applicable(s);
    case 5: return step5_applicable(s);
    default: return deep_applicable(s) && family_has_kernel(d, s->p.bc_mode);
    }
}

const int WORDS[] = {-1, 0, LB_VAR_STEP2, LB_VAR_STEP2 | LB_VAR_STEP3, LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4,
                     LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5,
                     LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5 | LB_VAR_STEP6,
                     LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5 | LB_VAR_STEP6 | LB_VAR_STEP7,
                     LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5 | LB_VAR_STEP6 | LB_VAR_STEP7 | LB_VAR_DEEP2,
                     LB_VAR_TILES, LB_VAR_STEP7, LB_VAR_STEP3 | LB_VAR_STEP6, LB_VAR_TILES | LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5};
const int SIZES[][2] = {{16, 12}, {63, 64}, {64, 64}, {256, 256}, {511, 300}, {512, 63}, {512, 64}, {512, 127}, {512, 128}, {514, 200}, {516, 200},
                        {1000, 1000}, {1024, 1024}, {1100, 1100}, {1280, 1280}, {1450, 1450}, {1500, 1500}, {1700, 1700}, {1900, 1900},
                        {2166, 2166}, {2900, 2900}, {3751, 1251}, {4096, 4096}, {8192, 8192}, {8192, 100}, {12288, 12288}};
const int NSIZES = (int)(sizeof(SIZES) / sizeof(SIZES[0]));

void sweep_plan_launches(Prop &p4, Prop &p7, Prop &p8)
{
    void check_hot_kernel(Prop &, const PlanInputs &);
    int d[256];
    for (int bc : FAMILIES)
        for (int si = 0; si < NSIZES; ++si)
            for (int word : WORDS)
                for (int tuned = 0; tuned <= MAX_DEPTH; ++tuned)
                    for (int wpc : {-1, 0, 4, 6, 8})
                        for (int bits = 0; bits < 4; ++bits) {
                            const int nx = SIZES[si][0], ny = SIZES[si][1];
                            if ((!tuned && wpc != 0) || (tuned && word >= 0)) continue;    // (lb_autotune's word counts only without the caller's)
                            if ((bits & 2) && nx < 8192) continue;                         // (the planar layout matters where planes stop fitting)
                            if (THIN && (si + tuned + bits) % 3) continue;
                            const int flags = (bits & 2) ? LB_FLAG_PLANAR : 0;
                            PlanInputs s = inputs(nx, ny, ny, bc, 256, LB_SEM_OPENCL, flags);
                            s.has_mask = bits & 1;
                            s.variant = word; s.tuned_steps = tuned; s.tuned_wpc = wpc;
                            if (tuned) s.depth_cost[tuned] = 0.5f + 0.1f * tuned;
                            const int allowed = whole_grid_depths(&s);
                            int deepest = 1;
                            for (int k = 2; k <= MAX_DEPTH; ++k)
                                if (allowed & (1 << k)) deepest = k;
                            for (int n = 0; n <= 200; n += n < 24 ? 1 : (n < 70 ? 5 : (n == 194 ? 6 : 31))) {       // (0 ... 24, 29 ... 69, 70, 101, 132, 163, 194, 200)
                                ++p4.cases;
                                const int c = plan_launches(&s, n, d, 256);
                                int sum = 0, mx = 0;
                                bool ok = c >= 0 && c <= 256 && c == plan_launches(&s, n, nullptr, 0);
                                for (int i = 0; ok && i < c; ++i) {
                                    sum += d[i]; mx = std::max(mx, d[i]);
                                    ok = d[i] >= 1 && d[i] <= MAX_DEPTH && depth_allowed_here(&s, d[i]) && !(d[i] >= 6 && bc == LB_BC_VELOCITY_INLET);
                                }
                                if (!ok || sum != n || (n == 200 && (mx != deepest || steps_per_launch(&s) != deepest)))
                                    p4.fail(fmt("bc %d %d x %d word %d tuned %d/%d mask %d flags %d, n = %d: %d launches summing to %d, deepest %d of %d (mask %#x)",
                                                bc, nx, ny, word, tuned, wpc, bits & 1, flags, n, c, sum, mx, deepest, allowed));
                            }
                            // P7: a plane too far for the marching kernels' 32-bit offsets leaves no marching depth
                            ++p7.cases;
                            if (!marching_planes_fit(&s) && !(allowed == 2 || (use_tile_kernel(&s) && allowed == depth_mask(false, false, true))))
                                p7.fail(fmt("bc %d %d x %d word %d flags %d: planes do not fit, whole_grid_depths %#x", bc, nx, ny, word, flags, allowed));
                            // P7: a remembered tuning result runs here only where launch_march has that kernel
                            if (!tuned)
                                for (int steps = 0; steps <= MAX_DEPTH + 1; ++steps)
                                    for (int w : {-1, 0, 2, 4, 6, 8}) {
                                        ++p7.cases;
                                        if (!tune_entry_runs_here(&s, steps, w)) continue;
                                        PlanInputs t = s;
                                        t.variant = -1; t.tuned_steps = steps; t.tuned_wpc = w;
                                        const int tw = whole_grid_depths(&t);
                                        const bool tiles = steps == 4 && w < 0;
                                        if (!family_has_kernel(steps, bc) || (tiles && (bc == LB_BC_VELOCITY_INLET || !use_tile_kernel(&t))) ||
                                            (steps >= 2 && !(tw & (1 << steps))) || (steps >= 2 && !tiles && !marching_planes_fit(&t)))
                                            p7.fail(fmt("bc %d %d x %d flags %d: tune entry %d steps / %d waves runs here, depths %#x", bc, nx, ny, flags, steps, w, tw));
                                    }
                            check_hot_kernel(p8, s);
                        }
    // every n = 0 ... 200 on one box per family, every word and every tuned depth
    for (int bc : FAMILIES)
        for (int word : WORDS)
            for (int tuned = 0; tuned <= MAX_DEPTH; ++tuned) {
                if (tuned && word >= 0) continue;
                PlanInputs s = inputs(2048, 2048, 2048, bc);
                s.variant = word; s.tuned_steps = tuned; s.tuned_wpc = tuned ? 8 : 0;
                if (tuned) s.depth_cost[tuned] = 0.5f + 0.1f * tuned;
                for (int n = 0; n <= 200; n += THIN ? 3 : 1) {
                    ++p4.cases;
                    const int c = plan_launches(&s, n, d, 256);
                    int sum = 0;
                    bool ok = c >= 0 && c <= 256;
                    for (int i = 0; ok && i < c; ++i) { sum += d[i]; ok = d[i] >= 1 && d[i] <= MAX_DEPTH && depth_allowed_here(&s, d[i]); }
                    if (!ok || sum != n) p4.fail(fmt("bc %d 2048 x 2048 word %d tuned %d, n = %d: %d launches summing to %d", bc, word, tuned, n, c, sum));
                }
            }
    // scalar lattices, the porous-medium fluid, Shan-Chen fluids, colonies: 4 a + r as tile launches then single steps, or single steps
    const int sems[] = {LB_SEM_DIFFUSION, LB_SEM_MULTIFIELD, LB_SEM_POISSON, LB_SEM_POROUS, LB_SEM_MULTIFLUID, LB_SEM_ROCKET};
    for (int sem : sems)
        for (int si = 0; si < NSIZES; ++si)
            for (int word : {-1, 0, 1, (int)LB_VAR_TILES, (int)LB_VAR_TILES | (3 << 2), (int)(LB_VAR_STEP2 | LB_VAR_STEP3 | LB_VAR_STEP4 | LB_VAR_STEP5 | LB_VAR_STEP6 | LB_VAR_STEP7)})
                for (int bc : {(int)LB_BC_PERIODIC, sem == LB_SEM_DIFFUSION ? (int)LB_BC_OPEN : sem == LB_SEM_MULTIFIELD ? (int)LB_BC_BOX
                                                    : sem == LB_SEM_POISSON ? (int)LB_BC_DIRICHLET : (int)LB_BC_ZERO_GRADIENT}) {
                    PlanInputs s = inputs(SIZES[si][0], SIZES[si][1], SIZES[si][1], bc, 256, sem);
                    s.variant = word;
                    const bool tiles = scalar_use_tiles(&s);
                    for (int n = 0; n <= 200; n += n < 24 ? 1 : 11) {
                        ++p4.cases;
                        const int c = plan_launches(&s, n, d, 256);
                        bool ok = tiles ? c == n / 4 + n % 4 : c == n;
                        for (int i = 0; ok && i < c; ++i) ok = d[i] == ((tiles && i < n / 4) ? TILE_T : 1);
                        if (!ok || steps_per_launch(&s) != (tiles ? TILE_T : 1) || (tiles && sem != LB_SEM_DIFFUSION))
                            p4.fail(fmt("semantics %d bc %d %d x %d word %d, n = %d: %d launches", sem, bc, SIZES[si][0], SIZES[si][1], word, n, c));
                    }
                    check_hot_kernel(p8, s);
                }
}

// ---- P5: next_advance ------------------------------------------------------------------------------------------------------------
void sweep_next_advance(Prop &p5, Prop &p5t)
{
    Rng rng(5);
    const int rounds = THIN ? 60 : 300;
    for (int round = 0; round < rounds; ++round) {
        // Costs on a grid of 1 / 64 between 0.25 and 2: every sum of up to 64 of them is exact in binary32 and in binary64, so
        // the split's cost must EQUAL the brute-force minimum, and ties are exact ties.  Every third round costs off the grid
        // (the seeds scaled by a random factor, jittered): there the sum of a split may lie above the minimum by what binary32
        // loses -- up to 64 additions of sums below 128, half an ulp (2^-17) each, = 4.9e-4 -- and by next_advance's own 1e-6 per
        // launch for a tie: bound 6e-4, against cost differences of 1e-2 and more.
        const bool exact = round % 5 == 0 ? round % 10 == 0 : round % 3 != 2;      // (the seeds themselves, every tenth round, are off the grid too)
        float cost[MAX_DEPTH + 1] = {0.f};
        static const float seed[MAX_DEPTH + 1] = {0.f, 0.79f, 0.85f, 0.89f, 0.86f, 0.96f, 1.00f, 1.08f};
        const float scale = 0.5f + rng.below(100) / 64.f;
        for (int k = 1; k <= MAX_DEPTH; ++k)
            cost[k] = exact ? (16 + rng.below(113)) / 64.f : seed[k] * scale * (0.9f + rng.below(2000) / 10000.f);
        if (round % 5 == 0)
            for (int k = 1; k <= MAX_DEPTH; ++k) cost[k] = round % 10 ? seed[k] : 1.f;       // the seeds themselves; all equal: ties everywhere
        const int allowed = 2 | (rng.below(64) << 2);
        int D = 1;
        for (int k = 2; k <= MAX_DEPTH; ++k)
            if (allowed & (1 << k)) D = k;
        // brute force: the cheapest split of m steps, and among the cheapest ones the deepest shallowest launch (the tie rule)
        double best[65];
        int shallowest[65];
        best[0] = 0.; shallowest[0] = 99;
        for (int m = 1; m <= 64; ++m) {
            best[m] = 1e300; shallowest[m] = 0;
            for (int k = 1; k <= std::min(m, MAX_DEPTH); ++k)
                if (k == 1 || (allowed & (1 << k))) best[m] = std::min(best[m], (double)cost[k] + best[m - k]);
            for (int k = 1; k <= std::min(m, MAX_DEPTH); ++k)
                if ((k == 1 || (allowed & (1 << k))) && (double)cost[k] + best[m - k] == best[m])
                    shallowest[m] = std::max(shallowest[m], std::min(k, shallowest[m - k]));
        }
        for (int left = 1; left <= 64; ++left) {
            ++p5.cases;
            double total = 0.;
            int l = left, launches = 0, prev = 0;
            bool ok = true, ascending = true;
            while (l > 0 && ok) {
                const int a = next_advance(allowed, l, cost);
                ok = a >= 1 && a <= l && (a == 1 || (allowed & (1 << a))) && ++launches <= 64;
                if (a < prev) ascending = false;
                prev = a;
                total += cost[a > 0 && a <= MAX_DEPTH ? a : 0];
                l -= a;
            }
            if (!ok || (exact ? total != best[left] : total > best[left] + 6e-4))
                p5.fail(fmt("allowed %#x left %d: the split costs %.6f, the cheapest %.6f", allowed, left, total, best[left]));
            if (exact) {
                ++p5t.cases;
                const int a = next_advance(allowed, left, cost);
                if (a != shallowest[left] || !ascending)
                    p5t.fail(fmt("allowed %#x left %d costs %.3f %.3f %.3f %.3f %.3f %.3f %.3f: first launch %d, the tie rule's %d%s", allowed, left, cost[1], cost[2], cost[3],
                                 cost[4], cost[5], cost[6], cost[7], a, shallowest[left], ascending ? "" : ", deeper launches first"));
            }
        }
        for (int left : {65, 66, 100, 1000, 1 << 30}) {
            ++p5.cases;
            if (next_advance(allowed, left, cost) != D) p5.fail(fmt("allowed %#x left %d: not the deepest depth %d", allowed, left, D));
        }
    }
}

// ---- P6: every rank of a run takes the same decisions; P7: what cycle_depth returns can run ------------------------------------------
void sweep_ranks(Prop &p6, Prop &p7)
{
    const int boxes[][2] = {{512, 512}, {1024, 1024}, {1280, 1280}, {1500, 1500}, {2048, 2048}, {2400, 2400}, {2600, 2600}, {3751, 1251}, {3800, 3800},
                            {4000, 4000}, {4096, 4096}, {8192, 8192}, {8192, 1024}, {12288, 12288}, {16384, 16384}, {1004, 9000}};
    const int cycle_words[] = {-1, 0, LB_VAR_STEP2 | LB_VAR_STEP3, WORDS[4], WORDS[5], WORDS[6], WORDS[7], WORDS[8], WORDS[7] | LB_VAR_NO_CYCLE, LB_VAR_STEP3 | LB_VAR_STEP5};
    Rng rng(6);
    for (const auto &box : boxes)
        for (int bc : FAMILIES)
            for (int ranks : {2, 3, 4, 8, 16, 64})
                for (int word : cycle_words)
                    for (int forced = 0; forced <= 8; forced += (forced == 0 ? 3 : 1))
                        for (int flavour = -1; flavour <= 1; ++flavour)
                            for (int transport = 0; transport <= 2; ++transport)
                                for (int planar = 0; planar < 2; ++planar) {
                                    const int nx = box[0], ny = box[1];
                                    if ((bc == LB_BC_PERIODIC && nx % 4) || ny / ranks < 16 || bc == LB_BC_VELOCITY_INLET) continue;      // (no slabs of that family: lb_create)
                                    if (THIN && ((forced * 7 + flavour + transport * 3 + planar + ranks) % 4)) continue;
                                    // (the smallest slab: an equal share, or a sixth of one beside taller slabs)
                                    const int min_h = (forced + flavour + transport) % 2 ? ny / ranks : std::max(16, ny / ranks / 6);
                                    const int max_h = ny - (ranks - 1) * min_h;
                                    int want[3] = {0, 0, 0};
                                    for (int r = 0; r < 6; ++r) {
                                        // a rank: its own height (the smallest one for r = 0), place, obstacles, GPU
                                        const int H = r == 0 ? min_h : (r == 1 ? max_h : min_h + rng.below(max_h - min_h + 1));
                                        PlanInputs s = inputs(nx, ny, H, bc, CUS[rng.below(4)], LB_SEM_OPENCL, LB_FLAG_HALO | (planar ? LB_FLAG_PLANAR : 0));
                                        s.p.y0 = r == 0 ? 0 : rng.below(ny - H + 1);
                                        s.has_mask = r & 1;
                                        if (r >= 4) s.lat_floats = r == 4 ? 1000 : (1LL << 33);        // (nothing of the cycle may hang on the bytes)
                                        s.min_h = min_h; s.nranks = ranks; s.variant = word; s.forced_cycle = forced; s.slab_flavour = flavour; s.transport = transport;
                                        const int got[3] = {cycle_depth(&s, min_h), slab_step_depths(&s, min_h), deep2_chosen(&s) ? 1 : 0};
                                        ++p6.cases;
                                        if (r == 0) memcpy(want, got, sizeof(got));
                                        else if (memcmp(want, got, sizeof(got)))
                                            p6.fail(fmt("bc %d %d x %d, %d ranks, word %d forced %d flavour %d transport %d: H %d mask %d gives cycle %d depths %#x deep2 %d, the "
                                                        "smallest rank %d %#x %d", bc, nx, ny, ranks, word, forced, flavour, transport, H, (int)s.has_mask, got[0], got[1], got[2], want[0], want[1], want[2]));
                                        // P7
                                        ++p7.cases;
                                        const int D = got[0], h = min_h;
                                        const int v = effective_variant(&s);
                                        // (its own threshold: 16 D rows -- the caller's depth as the automatic one --, 32 for the six-step cycle)
                                        const int floor_h = D >= 4 ? 16 * D : 32;
                                        if (D && (D < 3 || D > MAX_DEPTH || !step3_applicable(&s, h) || h < 32 || h < floor_h || !family_has_kernel(D, bc) || (v & LB_VAR_NO_CYCLE)))
                                            p7.fail(fmt("bc %d %d x %d min_h %d word %d forced %d: cycle depth %d cannot run", bc, nx, ny, h, word, forced, D));
                                        // (rows shared out evenly: the agreed plane is the slab's own, nothing is given up)
                                        if (max_h == min_h && marching_planes_fit(&s) != ((8.0 * (double)s.plane + (double)s.rowp) * 4.0 < 4294967296.0))
                                            p7.fail(fmt("bc %d %d x %d, %d even slabs: the planes' fit is not the slab's own", bc, nx, ny, ranks));
                                        if (!marching_planes_fit(&s) && (D || got[1] != 2))
                                            p7.fail(fmt("bc %d %d x %d H %d planar: planes do not fit, cycle %d, slab depths %#x", bc, nx, ny, H, D, got[1]));
                                        if ((got[1] & ~(2 | 4 | 8)) || ((got[1] & 4) && !step2_applicable(&s, h)) || ((got[1] & 8) && !step3_applicable(&s, h)))
                                            p7.fail(fmt("bc %d %d x %d min_h %d word %d: slab depths %#x", bc, nx, ny, h, word, got[1]));
                                    }
                                }
}

// ---- P8: hot_kernel ---------------------------------------------------------------------------------------------------------------
void check_hot_kernel(Prop &p8, const PlanInputs &s)
{
    char full[1024];
    memset(full, 0x7f, sizeof(full));
    hot_kernel(&s, full, (int)sizeof(full));
    ++p8.cases;
    if (!memchr(full, 0, sizeof(full))) { p8.fail("no terminator in 1024 bytes"); return; }
    // buffers of exactly 1, 8, 64 and 512 bytes on the heap (a byte past one is the sanitizer's to report): terminated inside, and
    // a prefix of the whole name
    for (int len : {1, 8, 64, 512}) {
        char *buf = (char *)malloc((size_t)len);
        memset(buf, 0x7f, (size_t)len);
        hot_kernel(&s, buf, len);
        ++p8.cases;
        const void *end = memchr(buf, 0, (size_t)len);
        if (!end) p8.fail(fmt("no terminator in a buffer of %d bytes", len));
        else {
            const size_t n = (size_t)((const char *)end - buf);
            // (the tuned suffix is appended by a second call and only where the first one fitted: a cut name is a prefix of the whole one)
            if (strncmp(buf, full, n) || (n < (size_t)len - 1 && n != strlen(full))) p8.fail(fmt("%d bytes: \"%s\" is no prefix of \"%s\"", len, buf, full));
        }
        free(buf);
    }
    // the name the plan implies
    std::string want;
    if (s.multifluid()) want = multifluid_one_launch(&s) ? "k_mc_step (" : "k_mc_moments + k_mc_collide (";
    else if (s.rocket()) want = rocket_one_launch(&s) ? "k_ry_step (" : "k_ry_moments + k_ry_collide (";
    else if (s.porous()) want = "k_pm_step (";
    else if (s.poisson()) want = "k_ps_step (";
    else if (s.multifield()) want = "k_mf_step (";
    else if (s.scalar()) want = scalar_use_tiles(&s) ? "k_ad_tile4 (" : "k_ad_step (";
    else if (s.p.semantics == LB_SEM_CYTHON) want = cython_tiles(&s) ? "k1_tile4 (" : "k1_fstep (";
    else {
        const int spl = steps_per_launch(&s);
        if (!s.multi_slab() && use_tile_kernel(&s) && spl == 4) want = "k_tile4 (";
        else if (spl == 7) want = deep2_chosen(&s) ? "k_deep2<7> (" : "k_deep<7> (";
        else if (spl == 6) want = "k_deep<6> (";
        else if (spl >= 2) want = fmt("k_step%d (", spl);
        else want = "k_step (";
    }
    ++p8.cases;
    if (strncmp(full, want.c_str(), want.size()))
        p8.fail(fmt("semantics %d bc %d %d x %d word %d tuned %d/%d: \"%.40s...\" where %s was due", s.p.semantics, s.p.bc_mode, s.p.nx, s.H, s.variant,
                    s.tuned_steps, s.tuned_wpc, full, want.c_str()));
    if (!s.scalar() && !s.porous() && !s.multifluid() && (strstr(full, ", MASK>") != nullptr) != s.has_mask) p8.fail(fmt("\"%.60s...\": the mask", full));
}

// slabs' names: the cycle's kernel
void sweep_hot_kernel_slabs(Prop &p8)
{
    for (int bc : FAMILIES)
        for (int word : WORDS)
            for (int flavour = -1; flavour <= 1; ++flavour)
                for (int transport = 0; transport <= 2; ++transport)
                    for (int H : {16, 40, 70, 100, 120, 512, 2048}) {
                        PlanInputs s = inputs(bc == LB_BC_PERIODIC ? 4096 : 4001, 4 * H, H, bc, 256, LB_SEM_OPENCL, LB_FLAG_HALO);
                        s.min_h = H; s.variant = word; s.slab_flavour = flavour; s.transport = transport;
                        check_hot_kernel(p8, s);
                    }
    for (int v : {-1, 0, (int)LB_VAR_TILES}) {
        PlanInputs s = inputs(96, 64, 64, LB_BC_PIPE, 256, LB_SEM_CYTHON);
        s.variant = v;
        check_hot_kernel(p8, s);
    }
}

// ---- xcd_item is a permutation of the workgroups (the decode above leans on it) ------------------------------------------------------
void sweep_xcd(Prop &px)
{
    std::vector<char> seen;
    for (int nwg = 1; nwg <= (THIN ? 700 : 2600); ++nwg) {
        ++px.cases;
        seen.assign((size_t)nwg, 0);
        bool ok = true;
        for (int wg = 0; wg < nwg && ok; ++wg) {
            const int i = xcd_item(wg, nwg);
            ok = i >= 0 && i < nwg && !seen[(size_t)i];
            if (ok) seen[(size_t)i] = 1;
        }
        if (!ok) px.fail(fmt("%d workgroups", nwg));
    }
}

// ---- --classify --------------------------------------------------------------------------------------------------------------------
// The class of the d-step launch of a whole grid (run_whole_grid: all rows; the velocity-inlet family: rows [d, ny - d), vel_band_pass):
//   seg_rows, the rows of the last interior segment, edge_seg_rows, the rows of the last wall segment (0: no split), the extra items,
//   items mod 64 and whether items >= 64, and the same of the workgroups, which are what xcd_item sees (k_step2 / k_step3: four
//   items each).
int classify(int nx, int ny, int bc, int depth)
{
    PlanInputs s = inputs(nx, ny, ny, bc, 256);
    if (!family_has_kernel(depth, bc) || depth < 2 || !step2_applicable(&s) || (depth >= 3 && !step3_applicable(&s))) {
        printf("none\n");
        return 2;
    }
    const int lo = bc == LB_BC_VELOCITY_INLET && depth >= 3 ? depth : 0, hi = ny - lo;
    const MarchPlan m = plan_march(&s, hi - lo, depth, MarchBands{}, 0);
    const int rows = hi - lo, extra = m.items - m.strips * m.segs;
    const int last_i = rows - (m.segs - 1) * m.seg_rows;
    const int last_e = m.edge_seg_rows ? rows - (m.segs + extra / 2 - 1) * m.edge_seg_rows : 0;
    const int wgs = depth >= 4 ? m.items : (m.items + 3) / 4;
    printf("seg_rows=%d last=%d edge_seg_rows=%d edge_last=%d extra=%d items=%d+%d%s wgs=%d+%d%s strips=%d segs=%d row_begin=%d\n", m.seg_rows, last_i, m.edge_seg_rows,
           last_e, extra, m.items % 64, 64 * (m.items / 64 > 0), m.items >= 128 ? "k" : "", wgs % 64, 64 * (wgs / 64 > 0), wgs >= 128 ? "k" : "", m.strips, m.segs, lo);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--classify")) return classify(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    // --onset nx bc depth: the smallest height at which the whole-grid launch splits its wall strips, and the smallest at which both
    // last segments of a split hold one row; the same two for a split whose wall segments are shorter than the interior's, i.e. with
    // extra items (how tests/march_shapes.py was drawn up)
    if (argc == 5 && !strcmp(argv[1], "--onset")) {
        const int nx = atoi(argv[2]), bc = atoi(argv[3]), depth = atoi(argv[4]);
        int onset = 0, ones = 0, shorter = 0, shorter_ones = 0;
        for (int ny = 128; ny <= 16384 && !(onset && ones && shorter && shorter_ones); ++ny) {
            PlanInputs s = inputs(nx, ny, ny, bc, 256);
            const int lo = bc == LB_BC_VELOCITY_INLET ? depth : 0, rows = ny - 2 * lo;
            const MarchPlan m = plan_march(&s, rows, depth, MarchBands{}, 0);
            if (!m.edge_seg_rows) continue;
            if (!onset) onset = ny;
            const int extra = m.items - m.strips * m.segs;
            const bool one_each = rows - (m.segs - 1) * m.seg_rows == 1 && rows - (m.segs + extra / 2 - 1) * m.edge_seg_rows == 1;
            if (!ones && one_each) ones = ny;
            if (!shorter && extra > 0) shorter = ny;
            if (!shorter_ones && extra > 0 && one_each) shorter_ones = ny;
        }
        printf("onset=%d ones=%d shorter=%d shorter_ones=%d\n", onset, ones, shorter, shorter_ones);
        return 0;
    }
    THIN = argc == 2 && !strcmp(argv[1], "--thin");
    if (argc > 1 && !THIN) {
        fprintf(stderr, "usage: plan_props [--thin | --classify nx ny bc depth | --onset nx bc depth]\n");
        return 2;
    }
    Prop p1("P1_coverage"), p1w("P1_width_only_through_strips"), p1b("P1_coverage_slab_launches"), p2("P2_one_round"), p3("P3_band_extra"), p4("P4_plan_launches"),
        p5("P5_next_advance"), p5t("P5_tie_rule"), p6("P6_rank_agreement"), p7("P7_consistency"), p8("P8_hot_kernel"), px("xcd_item_permutes");
    clock_t t0 = clock();
    auto lap = [&t0](const char *what) {                 // (where the time goes: stderr)
        const clock_t t1 = clock();
        fprintf(stderr, "%s: %.2f s\n", what, (double)(t1 - t0) / CLOCKS_PER_SEC);
        t0 = t1;
    };
    sweep_xcd(px); lap("xcd_item");
    sweep_balanced(p1, p2, p1w); lap("balanced launches");
    sweep_slabs(p1b, p3); lap("slab launches, band_extra");
    sweep_plan_launches(p4, p7, p8); lap("plan_launches, tuning entries, names");
    sweep_next_advance(p5, p5t); lap("next_advance");
    sweep_ranks(p6, p7); lap("ranks");
    sweep_hot_kernel_slabs(p8);
    int rc = 0;
    for (const Prop *p : {&px, &p1, &p1w, &p1b, &p2, &p3, &p4, &p5, &p5t, &p6, &p7, &p8}) rc |= p->report();
    return rc;
}
