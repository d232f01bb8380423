// tune.cpp -- lb_autotune / lb_autotune_quick: the candidate kernels timed on live steps, and what they found remembered across
// handles and processes (LB_TUNE_CACHE).
#include "host.h"

#include <climits>
#include <map>
#include <mutex>
#include <string>

namespace {

// ---- what lb_autotune found, remembered across handles and processes (opt-in: LB_TUNE_CACHE) ------------------------------------
// The kernel choice of a handle that was never tuned is a table of size thresholds measured on a pool of boxes that differ by +-5 %,
// and run(n) only tunes when n pays for it.  With LB_TUNE_CACHE=<file> (or "mem": this process only) every result of lb_autotune /
// lb_autotune_quick is stored under the handle's shape -- GPU, grid, rows owned, family, mask or not, layout, semantics -- and the
// first lb_run / lb_autotune_quick of a later handle of that shape takes it over (choice, waves per CU and the measured launch
// costs the launch plan is made from) without spending a step on tuning.  Every candidate is bitwise equivalent: only speed depends
// on it.  One text line per shape; a line that does not parse or names a kernel the handle cannot run is ignored.
struct TuneEntry { int steps, wpc; float cost[8]; };
std::mutex g_tune_mu;
std::map<std::string, TuneEntry> g_tune;
std::string g_tune_loaded_from;

const char *tune_cache_path()
{
    const char *e = getenv("LB_TUNE_CACHE");
    return (e && *e) ? e : nullptr;
}

std::string tune_key(const lb_sim *s)
{
    hipDeviceProp_t pr;
    char arch[64] = "gpu";
    int cus = 0;
    if (hipGetDeviceProperties(&pr, s->p.device) == hipSuccess) {
        snprintf(arch, sizeof(arch), "%s", pr.gcnArchName);
        for (char *c = arch; *c; ++c)
            if (*c == ' ' || *c == '\t') *c = '_';
        cus = pr.multiProcessorCount;
    }
    char k[256];
    snprintf(k, sizeof(k), "abi%d:%s:cu%d:%dx%d:rows%d:bc%d:mask%d:flags%x:sem%d", LB_ABI_VERSION, arch, cus, s->p.nx, s->p.ny, s->H,
             s->p.bc_mode, s->has_mask ? 1 : 0, (unsigned)s->p.flags, s->p.semantics);
    return k;
}

void tune_cache_load_locked(const char *path)
{
    if (g_tune_loaded_from == path) return;
    g_tune_loaded_from = path;
    if (strcmp(path, "mem") == 0) return;
    FILE *f = fopen(path, "r");
    if (!f) return;
    char key[256];
    TuneEntry e;
    while (fscanf(f, "%255s %d %d %f %f %f %f %f %f %f", key, &e.steps, &e.wpc, &e.cost[1], &e.cost[2], &e.cost[3], &e.cost[4], &e.cost[5],
                  &e.cost[6], &e.cost[7]) == 10) {
        e.cost[0] = 0.f;
        g_tune[key] = e;                                // (a later line of the same shape wins: the file is appended to)
    }
    fclose(f);
}

void tune_cache_store(const lb_sim *s)
{
    const char *path = tune_cache_path();
    if (!path || !s->tuned_steps) return;
    TuneEntry e;
    e.steps = s->tuned_steps;
    e.wpc = s->tuned_wpc;
    for (int d = 0; d < 8; ++d) e.cost[d] = d <= MAX_DEPTH ? s->depth_cost[d] : 0.f;
    const std::string key = tune_key(s);
    std::lock_guard<std::mutex> lock(g_tune_mu);
    tune_cache_load_locked(path);
    g_tune[key] = e;
    if (strcmp(path, "mem") == 0) return;
    if (FILE *f = fopen(path, "a")) {                   // (one short line per write: concurrent processes interleave whole lines)
        fprintf(f, "%s %d %d %.6g %.6g %.6g %.6g %.6g %.6g %.6g\n", key.c_str(), e.steps, e.wpc, e.cost[1], e.cost[2], e.cost[3], e.cost[4],
                e.cost[5], e.cost[6], e.cost[7]);
        fclose(f);
    }
}

}  // namespace

// takes over a remembered result; true if the handle is tuned afterwards
bool tune_cache_apply(lb_sim *s)
{
    s->tune_cache_checked = true;
    const char *path = tune_cache_path();
    if (!path || s->variant >= 0 || s->tuned_steps) return s->tuned_steps != 0;
    std::lock_guard<std::mutex> lock(g_tune_mu);
    tune_cache_load_locked(path);
    auto it = g_tune.find(tune_key(s));
    if (it == g_tune.end() || !tune_entry_runs_here(s, it->second.steps, it->second.wpc)) return false;
    s->tuned_steps = it->second.steps;
    s->tuned_wpc = it->second.wpc;
    for (int d = 0; d <= MAX_DEPTH; ++d) s->depth_cost[d] = d ? it->second.cost[d] : 0.f;
    return true;
}

namespace {

// Time the candidate configurations of the fused kernels on LIVE steps (every configuration produces
// bitwise identical results, so tuning advances the simulation like any other steps): four-, three- and
// two-step marching kernels at 8 and 4 waves per CU, and the single-step kernel.  Which one wins depends
// on the grid's aspect ratio, the mask and the boundary family (wide, short pipes favour fewer, longer
// segments: +20 % at 3751 x 1251).  Returns the number of steps advanced, or a negative status.  max_steps: the caller's budget --
// the rounds are the caller's to fit into it (autotune_quick_cost), the runner-up pass below is skipped where it would not fit.
int autotune_whole_grid(lb_sim *s, int rounds, int max_steps)
{
    struct Cand { int steps, wpc; };
    // (k_step4 at 8192^2 on one box: 4 waves per CU 189 k MLUPS, 6: 243 k, 8: 232 k, 12: 210 k -- profiles/r02_experiments.txt)
    // ({7, 8}: k_deep2<7>, the same march by two waves per strip and direction, eight waves per CU: the reference's 3751 x 1251 case 300
    //  against 293 k MLUPS, pipe 4096^2 409-423 against 400-407 k (profiles/r06l_reference_case_variants.txt, r06_deep2_check2.txt); periodic
    //  without a mask it depends on the box -- 8192^2 482-486 against 475-477 k and 4096^2 454-457 against 444-447 k on a middling one
    //  (profiles/r06u_deep2_headline.txt), 495-510 against 529 k on the fastest met -- which is what a tuner is for; it has to win by 1.5 %)
    const Cand cands[] = {{7, 4}, {7, 8}, {6, 4}, {5, 8}, {5, 6}, {4, 8}, {4, 6}, {4, 4}, {4, -1}, {3, 8}, {3, 6}, {3, 4}, {2, 8}, {2, 4}, {1, 0}};   // wpc -1: k_tile4
    // steps per timed sample: 3 x 4 = 4 x 3 = 6 x 2 = 12 x 1 (the five-step candidates: 2 x 5; compared by time per step);
    // small grids: 36, so that the single-step candidate runs the way it would (hipGraph replay of 16 launches)
    const int per12 = small_grid(s) ? 36 : 12;
    auto per_of = [&](const Cand &c) { return c.steps == 5 ? 10 : (c.steps == 7 ? 14 : per12); };
    const int keep_steps = s->tuned_steps, keep_wpc = s->tuned_wpc;
    int used = 0, best = -1;
    float best_ms = 0.f;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // any failure: events destroyed, the previous choice restored (the steps taken so far stay taken -- they are
    // ordinary time steps)
    auto bail = [&](int rc) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        s->tuned_steps = keep_steps;
        s->tuned_wpc = keep_wpc;
        return rc;
    };
#define TUNE_TRY(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return bail(fail(LB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__)); \
    } while (0)
    TUNE_TRY(hipEventCreate(&e0));
    TUNE_TRY(hipEventCreate(&e1));
    // Rounds outside, candidates inside: round 0 warms every configuration (and the device: on a GPU that has just been
    // initialised the clocks are still ramping, and with the candidates sampled one after the other the first one -- four
    // steps at 8 waves per CU, the usual winner -- lost to the second by that alone: 283 k instead of 309 k MLUPS at 8192^2
    // for everything run after a quick tune; profiles/r02_experiments.txt), the later rounds are compared by their minimum.
    constexpr int NC = (int)(sizeof(cands) / sizeof(cands[0]));
    float ms_min[NC];
    bool usable[NC];
    for (int c = 0; c < NC; ++c) {
        ms_min[c] = 0.f;
        usable[c] = !(cands[c].steps >= 6 && !deep_applicable(s)) && !(cands[c].steps == 5 && !step5_applicable(s)) &&
                    !(cands[c].steps == 4 && cands[c].wpc >= 0 && !step4_applicable(s)) && !(cands[c].wpc < 0 && !tile_applicable(s)) &&
                    !(cands[c].steps == 3 && !step3_applicable(s)) && !(cands[c].steps == 2 && !step2_applicable(s));
    }
    for (int r = 0; r <= rounds; ++r) {
        for (int c = 0; c < NC; ++c) {
            if (!usable[c]) continue;
            s->tuned_steps = cands[c].steps;
            s->tuned_wpc = cands[c].wpc;
            TUNE_TRY(hipEventRecord(e0, s->stream));
            const int per = per_of(cands[c]);
            int rc = run_whole_grid(s, per, false);     // no rho,u,v epilogue: it would weigh on the short samples
            if (rc) return bail(rc);
            TUNE_TRY(hipEventRecord(e1, s->stream));
            TUNE_TRY(hipEventSynchronize(e1));
            float ms = 0.f;
            TUNE_TRY(hipEventElapsedTime(&ms, e0, e1));
            ms /= (float)per;                           // time per step
            used += per;
            if (r >= 1 && (r == 1 || ms < ms_min[c])) ms_min[c] = ms;
        }
    }
    for (int c = 0; c < NC; ++c)
        if (usable[c] && (best < 0 || ms_min[c] < best_ms)) { best = c; best_ms = ms_min[c]; }
    // A runner-up within 5 % (round 5: k_step5 and k_deep<7> on config 5, 19.7 against 19.1 steps per ms -- the choice flipped from run to
    // run, the rocprofv3 profile and the driver's line named different kernels): the two once more over samples four times as long, three
    // rounds alternating, minimum of each.  Only where the caller's budget holds it and the closing step below: 3 x 4 x (14 + 14) = 336
    // steps for the two seven-step kernels, which lb_autotune_quick(h, 361) has no room for (its rounds alone take up to 360 + 1).
    if (best >= 0 && !small_grid(s)) {
        int second = -1;
        for (int c = 0; c < NC; ++c)
            if (usable[c] && c != best && (cands[c].steps != cands[best].steps || cands[c].steps == 7) &&       // (7: k_deep<7> against k_deep2<7>)
                (second < 0 || ms_min[c] < ms_min[second])) second = c;
        if (second >= 0 && ms_min[second] < 1.05f * best_ms &&
            3 * 4 * (per_of(cands[best]) + per_of(cands[second])) <= max_steps - used - 1) {
            float again[2] = {1e30f, 1e30f};
            const int pair[2] = {best, second};
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 2; ++k) {
                    const Cand &cd = cands[pair[k]];
                    s->tuned_steps = cd.steps;
                    s->tuned_wpc = cd.wpc;
                    const int per = 4 * per_of(cd);
                    TUNE_TRY(hipEventRecord(e0, s->stream));
                    int rc = run_whole_grid(s, per, false);
                    if (rc) return bail(rc);
                    TUNE_TRY(hipEventRecord(e1, s->stream));
                    TUNE_TRY(hipEventSynchronize(e1));
                    float ms = 0.f;
                    TUNE_TRY(hipEventElapsedTime(&ms, e0, e1));
                    used += per;
                    again[k] = std::min(again[k], ms / (float)per);
                }
            ms_min[best] = again[0];
            ms_min[second] = again[1];
            if (again[1] < again[0]) best = second;
            best_ms = ms_min[best];
        }
    }
#undef TUNE_TRY
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
    // (k_deep2<7> has to be ahead of k_deep<7> by more than the samples scatter: 1.5 %)
    if (best >= 0 && cands[best].steps == 7 && cands[best].wpc == 8 && usable[0] && ms_min[0] <= 1.015f * ms_min[best]) {
        best = 0;
        best_ms = ms_min[0];
    }
    if (best < 0) return bail(0);                       // nothing applicable
    s->tuned_steps = cands[best].steps;
    s->tuned_wpc = cands[best].wpc;
    // what a launch of each depth costs on this handle (next_advance splits runs by it): the winner's time for its depth; for the
    // others the candidate they will be launched as -- eight waves per CU (k_deep: four), the tiles or not as the winner
    for (int d = 0; d <= MAX_DEPTH; ++d) s->depth_cost[d] = 0.f;
    for (int c = 0; c < NC; ++c) {
        if (!usable[c] || small_grid(s)) continue;      // (small grids replay single steps from a graph: the sample is not a launch)
        const Cand &k = cands[c];
        const bool as_launched = (c == best) || (k.steps != cands[best].steps && !(k.steps == 7 && k.wpc == 8) &&
                                                 (k.steps >= 6 || k.steps == 1 || (k.steps == 4 && cands[best].wpc < 0 ? k.wpc < 0 : k.wpc == 8)));
        if (as_launched) s->depth_cost[k.steps] = ms_min[c] * (float)k.steps;
    }
    // one more step that stores rho,u,v so that the observable state is consistent again
    int rc = launch_step(s, 0, 1, s->H, true);
    if (rc) return rc;
    s->cur ^= 1;
    s->feq_valid = false;
    s->macro_valid = !lazy_macro(s);
    tune_cache_store(s);
    return used + 1;
}

// steps a quick (one-round) tuning pass consumes at most: 11 candidates x 2 samples x 12 (36) steps, 2 x 2 x 10, 2 x 2 x 14, + 1
// (an upper bound: every candidate usable).  The runner-up pass of autotune_whole_grid is not counted: it only runs where the
// budget it is given holds it, and lb_autotune_quick gives it max_steps, so the quick pass never advances more than max_steps.
int autotune_quick_cost(const lb_sim *s) { return 11 * 2 * (small_grid(s) ? 36 : 12) + 2 * 2 * 10 + 2 * 2 * 14 + 1; }

}  // namespace

extern "C" {

int lb_autotune(lb_sim *s)
{
    if (s && s->cpu) return 0;                     // (one code path on the host: nothing to choose between)
    SCALAR_UNSUPPORTED(s, "lb_autotune");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_autotune inside a split step");
    if (!autotune_applies(s)) return 0;                // nothing to choose between
    // (a forced variant fixes the kernels: every candidate would be timed as those, and the launch plan made from such costs is
    //  nonsense -- bench.py --variant 119137 (LB_VAR_DEEP2 and every marching bit) planned twenty steps as 1 + 1 + 4 + 7 + 7)
    if (s->variant >= 0) return 0;
    // (LB_TUNE_CACHE holds a result for this shape: taken over, as lb_autotune_quick and lb_run do -- a profiled run then names the
    //  kernel the un-profiled run before it chose: tools/gpu_profile.sh)
    if (!s->tune_cache_checked && s->variant < 0 && !s->tuned_steps && tune_cache_apply(s)) return 0;
    DeviceGuard guard(s->p.device);
    return autotune_whole_grid(s, 6, INT_MAX);        // (unbounded: the runner-up pass always runs when it applies)
}

int lb_autotune_quick(lb_sim *s, int max_steps)
{
    if (s && s->cpu) return 0;
    SCALAR_UNSUPPORTED(s, "lb_autotune_quick");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_autotune_quick inside a split step");
    if (!s->tune_cache_checked && tune_cache_apply(s)) return 0;       // (LB_TUNE_CACHE: an earlier handle of this shape was tuned)
    if (!autotune_applies(s) || s->variant >= 0 || s->tuned_steps || max_steps < autotune_quick_cost(s)) return 0;
    DeviceGuard guard(s->p.device);
    return autotune_whole_grid(s, 1, max_steps);
}

}  // extern "C"
