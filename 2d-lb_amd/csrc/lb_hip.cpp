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
// k_step5), kernels_deep.h (k_deep: six and seven steps per pass), kernels_tile.h (k_tile4, k_vel_band), kernels_phases.h (un-fused phases, halo pack / unpack, peer transport);
// every fused kernel family is instantiated in a translation unit of its own (launchers.h), this file holds the RCCL loader,
// the host side, the C ABI and the small kernels of kernels_phases.h.
// All stores of the fused kernel are 16-byte aligned; the six planes with cx != 0 are read through
// 16-byte loads that are misaligned by one element (gfx950 global loads only need dword alignment).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>
#include <unistd.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lb_hip.h"
#include "cpu_backend.h"

namespace {

constexpr int GHOST = 14;  // ghost rows below row 0 and above row H-1 of every plane: a slab runs two seven-step
                           // launches per halo exchange, the first one recomputing 7 of the neighbour's rows
constexpr int MASK_GHOST = LB_MASK_HALO_ROWS;   // mask rows kept of each neighbouring slab (step 1 of row -13)
constexpr int GUARD = 512; // floats in front of / behind each lattice allocation (the marching kernels' last
                           // strip reads up to 257 cells past a row's end, every kernel 1 cell before its start)

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(LB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                                   \
    } while (0)

}  // namespace

#include "d2q9_cell.h"
#include "kernels_fused.h"
#include "kernels_step4.h"
#include "kernels_step5.h"
#include "kernels_deep.h"
#include "kernels_tile.h"
#include "kernels_phases.h"
#include "launchers.h"          // the fused kernels are instantiated in their own translation units

namespace {

// ------------------------------------------------------------------------------------------
//  RCCL, loaded lazily so that single-GPU use never touches librccl
// ------------------------------------------------------------------------------------------
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
} g_rccl;

int rccl_load()
{
    if (g_rccl.lib) return LB_OK;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(LB_ERR_COMM, "cannot load librccl.so: %s", dlerror());
#define SYM(field, name)                                                                     \
    *(void **)(&g_rccl.field) = dlsym(h, name);                                              \
    if (!g_rccl.field) return fail(LB_ERR_COMM, "librccl.so lacks %s", name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(AllReduce, "ncclAllReduce");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.lib = h;
    return LB_OK;
}

#define NCCL_TRY(expr)                                                                        \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail(LB_ERR_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));      \
    } while (0)

}  // namespace

// ------------------------------------------------------------------------------------------
//  host side
// ------------------------------------------------------------------------------------------
struct lb_sim {
    lb_params p;
    lbcpu::CpuPipe *cpu = nullptr;   // device = LB_DEVICE_CPU: the host backend (cpu_backend.h); every device member below stays empty
    int H = 0;                  // rows owned
    long long pitch = 0, rowp = 0, plane = 0, lat_floats = 0;   // padded row width; lattice row / plane strides; floats per lattice
    float *lat[2] = {nullptr, nullptr};   // raw allocations (with guards)
    int cur = 0;                // lattice holding f
    int stepping = 0;           // 1 between lb_step_boundary and lb_step_finish
    float *feq = nullptr;       // raw allocation, lazily created
    float *rho = nullptr, *u = nullptr, *v = nullptr;
    float *stage = nullptr;     // [H][pitch], lazily: one plane on its way between the host and interleaved rows (lattice_plane_*)
    float *vi_corner = nullptr; // VELOCITY_INLET: the eight corner links nothing ever writes (bc_vel_cell), device
    uint8_t *mask_raw = nullptr, *mask = nullptr;   // [H+2*MASK_GHOST][pitch] + guards; mask -> row 0
    bool has_mask = false;
    int cu_count = 256;
    bool feq_valid = false;     // feq buffer consistent with rho,u,v
    bool macro_valid = true;    // rho,u,v hold the last step's fields (false: to be rebuilt from the populations, ensure_macro)
    CheckPartial *check_part = nullptr;   // one partial per workgroup of k_macro_check (+ the folded result behind them)
    long long check_cap = 0;
    hipStream_t own_stream = nullptr, stream = nullptr, comm_stream = nullptr, edge_stream = nullptr;
    hipEvent_t ev_boundary = nullptr, ev_interior = nullptr, ev_halo = nullptr, ev_packed = nullptr, ev_edge = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    int min_h = 0;              // smallest slab height over the ranks (every rank must pick the same schedule)
    float *halo_buf = nullptr;  // 4 x HALO_SEGS_DEEP (117) x nx floats: send north, send south, recv south, recv north
    int ghost_depth = 0;        // ghost rows of lat[cur] hold this many of the neighbours' edge rows (0, 3, 6 or 8)
    int variant = -1;           // < 0: automatic (effective_variant)
    hipGraph_t graph = nullptr;            // GRAPH_STEPS single-step launches, captured for small grids
    hipGraphExec_t graph_exec = nullptr;
    int graph_key = -1;                    // state the capture is valid for (cur, mask, variant)
    hipStream_t graph_stream = nullptr;
    bool graph_failed = false;
    // peer transport (lb_peer_export / lb_peer_connect): my flag block, the neighbours' flag blocks and lattices as mapped here
    unsigned long long *peer_flags = nullptr;
    bool peer_flags_fine = false;
    bool peer_connected = false;
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
    int slab_flavour = -1;      // slabs, seven-step cycle: 0 k_deep<7>, 1 k_deep2<7> (lb_set_slab_cycle(8)), -1 automatic (k_deep2 under RCCL)
    int forced_cycle = 0;       // slabs: depth of the fused kernel the halo cycle runs on, fixed by the caller (lb_set_slab_cycle); 0 = automatic
    // lb_exchange_timing: a pair of timing events around every halo exchange of lb_run, on the stream that carries it
    static constexpr int XT_RING = 256;
    bool xt_on = false;
    hipEvent_t xt_ev[2 * XT_RING] = {};
    int xt_count = 0, xt_dropped = 0;
    int tuned_steps = 0;        // 0: not tuned; else the fused kernel depth (1..4) chosen by lb_autotune
    int tuned_wpc = 0;          // and its waves per CU for the marching kernels
    float depth_cost[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // ms per launch of the d-step kernel as lb_autotune timed it (0: not timed): launch_costs
    bool tune_cache_checked = false;    // LB_TUNE_CACHE has been consulted for this handle's present shape (lb_set_mask resets it)
    int64_t bytes = 0;

    float *origin(int which) const { return lat[which] + GUARD + GHOST * rowp; }   // plane 0, row 0, x 0
    float *feq_origin() const { return feq + GUARD + GHOST * rowp; }
    bool multi_slab() const { return H != p.ny || (p.flags & LB_FLAG_HALO); }
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Handles of the CPU backend: an entry point either has a host form or refuses.
#define CPU_UNSUPPORTED(s, name)                                                                            \
    do {                                                                                                    \
        if ((s) && (s)->cpu) return fail(LB_ERR_STATE, "%s is not available on the CPU backend", name);      \
    } while (0)

// boundary family as the kernels' template argument (the D2Q9i fork is the PIPE family with its own cell routines)
int kernel_bc(const lb_sim *s) { return s->p.semantics == LB_SEM_OPENCL_D2Q9I ? LB_BC_PIPE_I : s->p.bc_mode; }

// rho, u, v of the plain families are rebuilt from the populations on demand instead of being stored by the last launch
// of every run (include/lb_hip.h, LB_FLAG_EAGER_MACRO); LB_EAGER_MACRO=1 in the environment = the flag on every handle
bool lazy_macro(const lb_sim *s)
{
    static const bool eager_env = getenv("LB_EAGER_MACRO") && atoi(getenv("LB_EAGER_MACRO")) != 0;
    return !eager_env && !(s->p.flags & LB_FLAG_EAGER_MACRO) && s->p.semantics == LB_SEM_OPENCL &&
           (s->p.bc_mode == LB_BC_PIPE || s->p.bc_mode == LB_BC_PERIODIC || s->p.bc_mode == LB_BC_CAVITY);
}

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
    a.tile_launch_order = (s->variant >= 0 && (s->variant & VAR_TILE_LAUNCH_ORDER)) ? 1 : 0;    // (A/B switch: explicit variants only)
    a.diag = s->diag;
    a.prio_turns = 0;      // (set by launch_step2 from the variant)
    a.nts = 0;
    a.omega = s->p.omega; a.rho_in = s->p.inlet_rho; a.rho_out = s->p.outlet_rho;
    a.lid_u = s->p.lid_u; a.rho0 = s->p.rho0;
    return a;
}

// variant < 0 = automatic, from one-GPU sweeps (tools/sweep.py, tools/rect_probe.py;
// profiles/r01_sweep_variants.txt):
//   >= 1024^2 / 1280^2 cells on this GPU : temporal blocking -- three / four time steps per pass (marching
//                                          kernels; nx >= 512 and enough rows, else they do not apply)
//   lattice pair >= 450 MB (3072^2 up)   : + non-temporal stores (+3..10 %), and 4 rows x 256 cells per
//                                          workgroup wherever the single-step kernel runs (with contiguous
//                                          planes 2 x 512 was the better shape; with interleaved rows 4 x 256
//                                          streams 3..8 % faster at 4096^2 / 8192^2: profiles/r02_experiments.txt)
//   smaller (Infinity-Cache resident)    : single step, plain stores, XCD-aware tile order
int effective_variant(const lb_sim *s)
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
    int v = pair_bytes >= 3.2e8 ? ((s->p.flags & LB_FLAG_PLANAR) ? VAR_NT_STORES | VAR_ROWS_2 : VAR_NT_STORES) : VAR_XCD_ORDER;
    // from 1024^2 cells: three steps per pass (110 k MLUPS at 1024^2 against 87 k single-step); from 1280^2:
    // four (125 k at 1280^2, 158 k at 1536^2, 170 k at 2048^2, 220 k from 3072^2), whole grids and slabs alike,
    // in every boundary family, with and without obstacles (profiles/r01_sweep_variants.txt,
    // profiles/r01_slab_proxy_1gpu.txt).  Smaller grids: single step, replayed through a hipGraph.
    if (cells >= 1024.0 * 1024.0) v = (v & ~VAR_XCD_ORDER) | VAR_STEP2 | VAR_STEP3;
    if (cells >= 1280.0 * 1280.0) v |= VAR_STEP4;
    // ... and five wherever four are (k_step5, overlapping strips: periodic 2048^2 298 against 250 k MLUPS, 4096^2 315 against 289 k,
    // 8192^2 327-346 against 306-319 k; pipe 8192^2 346 against 309 k: profiles/r04_experiments.txt section 10), in every family,
    // whole grids and slabs (cycle_depth) alike
    if (cells >= 1280.0 * 1280.0) v |= VAR_STEP5;
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
        v |= VAR_STEP6 | VAR_STEP7;     // (slabs: inside the twelve- / fourteen-step halo cycle, cycle_depth)
        if (whole_grid && !s->multi_slab() && !periodic_box && cells < 2900.0 * 2900.0) v |= VAR_DEEP2;
    }
    // Periodic whole grids without a mask, tiles | k_step5 | k_deep<6> | k_deep<7>, k MLUPS, 1680-step runs (profiles/r06q_periodic_small_sweep.txt):
    // 1024^2 214 | 186 | 205 | 195, 1152^2 220 | 227 | 246 | 239, 1280^2 234 | 256 | 263 | 258, 1408^2 242 | 266 | 291 | 287, 1536^2 245 | 291 | 310 | 308,
    // 1792^2 254 | 319 | 364 | 359, 2048^2 210 | 293 | 340 | 364: six steps per pass from 1100^2 cells, seven from 1900^2 (use_tile_kernel:
    // the tiles below 1100^2).
    if (periodic_box && whole_grid && !s->multi_slab() && !s->has_mask) {
        v &= ~(VAR_STEP6 | VAR_STEP7);
        if (cells >= 1100.0 * 1100.0) v |= VAR_STEP4 | VAR_STEP5 | VAR_STEP6;
        if (cells >= 1900.0 * 1900.0) v |= VAR_STEP7;
    }
    return v;
}

// Launch the fused step over local rows row_begin + i*row_step, i < row_count.
int launch_step(lb_sim *s, int row_begin, int row_step, int row_count, bool macro)
{
    if (row_count <= 0) return LB_OK;
    macro = macro && !lazy_macro(s);       // (no fused kernel stores rho, u, v on a handle that rebuilds them on demand)
    const StepArgs a = step_args(s, row_begin, row_step, row_count);
    const int variant = effective_variant(s);
    const int rpb_sel = variant & VAR_ROWS;
    const int rows_per_block = rpb_sel == VAR_ROWS_1 ? 1 : (rpb_sel == VAR_ROWS_2 ? 2 : 4);
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
// instantiation without an obstacle mask but the D2Q9i fork's); VAR_STEP4_NO_AHEAD switches it off (A/B runs).
bool deep2_chosen(const lb_sim *s)
{
    if (s->multi_slab() && s->slab_flavour >= 0) return s->slab_flavour == 1;      // lb_set_slab_cycle(7) / (8): the caller's word
    if (s->variant >= 0) return (s->variant & VAR_DEEP2) != 0;
    // Slabs without the caller's word (above: the ranks' collective tuner): by transport.  Beside k_deep<7> (2 x 80 KB of
    // LDS per CU, lone waves) RCCL's send / receive kernel waits for places and slows what it shares SIMDs with; k_deep2<7>'s launches
    // (2 x 72 KB, waves in pairs per SIMD) do not run longer for it, though it still takes most of a launch beside them: one slab of 4 | 2 of an 8192^2 lattice over RCCL 381-392 | 402-450 k MLUPS by k_deep, 443-444 | 466 k by
    // k_deep2 = the peer transport's rate; of 8: 374-381 | 383-392; the peer transport itself: equal within 1 %
    // (profiles/r06s_slab_proxy_deep2.txt).  Every rank of a run shares the transport, so the ranks agree.
    if (s->multi_slab()) return s->comm != nullptr && !s->peer_connected;
    if (s->tuned_steps) return s->tuned_steps == 7 && s->tuned_wpc == 8;       // lb_autotune's word
    return (effective_variant(s) & VAR_DEEP2) != 0;                                // the size table's
}

bool launch_march(const lb_sim *s, hipStream_t st, const StepArgs &a, int items, int strips, int seg_rows, int nsegs, int row_end,
                  bool macro, int depth)
{
    const int waves = (depth >= 4) ? STEP4_WAVES : 4;      // waves per workgroup: k_step4 ... k_step6: the two directions of ONE item
                                                           // (a segment pair); the others: four independent items
    MarchLaunch g;
    g.block = dim3(64, waves);
    g.grid = dim3(depth >= 4 ? items : (items + waves - 1) / waves);
    g.stream = st;
    g.strips = strips; g.seg_rows = seg_rows; g.nsegs = nsegs; g.row_end = row_end;
    const int bc = kernel_bc(s);
    // (false: the unit has no instantiation for this boundary family -- k_deep / k_deep2 and the velocity-inlet family)
    // k_deep2: four waves per workgroup -- asked for (VAR_DEEP2) or found faster by lb_autotune (seven steps at "eight waves per CU")
    if (depth == 7 && deep2_chosen(s)) return lbk_launch_deep2_7(bc, s->has_mask, macro, g, a);
    if (depth == 7) return lbk_launch_deep7(bc, s->has_mask, macro, g, a);
    if (depth == 6) return lbk_launch_deep6(bc, s->has_mask, macro, g, a);
    if (depth == 5) lbk_launch_march5(bc, s->has_mask, macro, g, a);
    else if (depth == 4) lbk_launch_march4(bc, s->has_mask, macro, !(effective_variant(s) & VAR_STEP4_NO_AHEAD), g, a);
    else lbk_launch_march23(depth, bc, s->has_mask, macro, g, a);
    return true;
}

// The marching kernels address the nine planes of a row through ONE scalar base and a 32-bit byte offset per lane that carries the
// plane (store_row9): (x + 8 plane) * 4 must stay below 4 GB.  Always true for the default layout (plane = the padded row);
// LB_FLAG_PLANAR lattices of more than ~11000^2 cells take the single-step kernel and the tiles instead.
bool marching_planes_fit(const lb_sim *s) { return (8.0 * (double)s->plane + (double)s->rowp) * 4.0 < 4294967296.0; }

// (h: the height the decision is taken on -- a slab's own, or the smallest of the slabs that must agree)
bool step3_applicable(const lb_sim *s, int h = -1)
{
    if (h < 0) h = s->H;
    if (!marching_planes_fit(s)) return false;
    if (s->p.nx < 512 || h < (s->multi_slab() ? 32 : 128)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// four steps per pass on a whole-grid handle (slabs use it inside the eight-step halo cycle only: cycle_depth)
bool step4_applicable(const lb_sim *s)
{
    if (s->multi_slab() || s->p.nx < 512 || s->H < 128 || !marching_planes_fit(s)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// five steps per pass (k_step5) on a whole-grid handle (slabs: inside the ten-step halo cycle, cycle_depth)
bool step5_applicable(const lb_sim *s) { return step4_applicable(s); }
// six / seven steps per pass (k_deep): whole-grid handles; not the velocity-inlet family (its wall-row bands stop at five)
bool deep_applicable(const lb_sim *s) { return step4_applicable(s) && s->p.bc_mode != LB_BC_VELOCITY_INLET; }
constexpr int MAX_DEPTH = 7;            // deepest fused kernel

// four steps per pass through LDS tiles (k_tile4): whole-grid handles, any width
bool tile_applicable(const lb_sim *s)
{
    return s->p.bc_mode != LB_BC_VELOCITY_INLET && !s->multi_slab() &&
           s->p.nx >= 64 && s->H >= 64;
}

bool step2_applicable(const lb_sim *s, int h = -1)
{
    if (h < 0) h = s->H;
    if (s->p.nx < 512 || !marching_planes_fit(s)) return false;
    if (h < (s->multi_slab() ? 16 : 64)) return false;
    if (s->p.bc_mode == LB_BC_PERIODIC && (s->p.nx % 4) != 0) return false;
    return true;
}

// Output rows [row_begin, row_end) in `nsegs_fixed` segments of seg_rows_fixed rows spaced seg_stride
// apart (edge bands), or -- nsegs_fixed == 0 -- cut into equal shares so that the launch is one
// balanced round of resident waves (reserve = wave slots left to a concurrent edge launch).
int launch_step2(lb_sim *s, hipStream_t st, int row_begin, int row_end, bool macro, int nsegs_fixed = 0,
                 int seg_rows_fixed = 0, int seg_stride = 0, int reserve = 0, int depth = 2)
{
    if (row_end <= row_begin) return LB_OK;
    macro = macro && !lazy_macro(s);
    StepArgs a = step_args(s, row_begin, 1, row_end - row_begin);
    const int variant = effective_variant(s);
    // (k_step5: overlapping strips, 248 cells apart)
    const int strips = depth >= 6 ? deep_strips(s->p.nx, depth) : (depth == 5 ? step5_strips(s->p.nx) : (s->p.nx + STRIP_W - 1) / STRIP_W);
    int segs, seg_rows, extra_items = 0;
    if (nsegs_fixed > 0) {
        segs = nsegs_fixed;
        seg_rows = seg_rows_fixed;
        a.seg_stride = seg_stride;
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
        const int rows = row_end - row_begin;
        segs = capacity / strips;
        if (segs < 1) segs = 1;
        seg_rows = (rows + segs - 1) / segs;
        // (floor: grids of 1024^2 .. 2048^2 are latency-bound, not bandwidth-bound -- filling every wave slot
        //  with a short segment beats fewer, longer ones although each segment recomputes (d-1) [k_step4] or 2(d-1) rows:
        //  with the earlier floor of 16 rows 2048^2 ran at 142 k MLUPS, with 4..8 at 170 k: profiles/r01_sweep_variants.txt)
        if (seg_rows < 4 * per_item) seg_rows = 4 * per_item;
        segs = (rows + seg_rows - 1) / seg_rows;
        a.seg_stride = seg_rows;
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
        const double edge_cost = s->p.bc_mode == LB_BC_VELOCITY_INLET ? (depth == 5 ? 2.3 : 1.6) : (depth >= 6 ? 2.1 : 1.2);
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
                a.seg_stride = rows_i;
                a.edge_seg_rows = rows_e;
                extra_items = 2 * ((rows + rows_e - 1) / rows_e - segs);
                if (extra_items < 0) extra_items = 0, a.edge_seg_rows = 0;
            }
        }
    }
    const int items = strips * segs + extra_items;
    const bool nts = (variant & VAR_NT_STORES) != 0;
    // k_step4: the two waves of a SIMD take turns at the higher issue priority (see the kernel), in turns of 2^13 ticks of the 100 MHz clock; VAR_NO_PRIO_TURNS = off
    a.prio_turns = (variant & VAR_NO_PRIO_TURNS) ? 0 : 13;
    a.nts = nts ? 1 : 0;                       // (the marching kernels take it at run time)
    if (!launch_march(s, st, a, items, strips, seg_rows, segs, row_end, macro, depth))
        return fail(LB_ERR_STATE, "no %d-step kernel for this boundary family (the caller's schedule must not ask for one)", depth);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// which of k_tile4's three shapes (launchers.h: lbk_launch_tile4)
int tile_shape_of(const lb_sim *s)
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

// Four time steps of a whole-grid handle through LDS tiles.
int launch_tile4(lb_sim *s, bool macro)
{
    macro = macro && !lazy_macro(s);
    const StepArgs a = step_args(s, 0, 1, s->H);
    if (!lbk_launch_tile4(kernel_bc(s), s->has_mask, macro, tile_shape_of(s), s->p.nx, s->H, s->stream, a))
        return fail(LB_ERR_STATE, "no LDS-tile kernel for this boundary family");
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

constexpr int GRAPH_STEPS = 16;

bool small_grid(const lb_sim *s) { return (double)s->p.nx * s->H <= 768.0 * 768.0; }

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
int ensure_graph(lb_sim *s)
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

// One pass over the current populations (k_macro_check): store = rebuild rho, u, v from them; the per-workgroup partials of
// the health check are folded into check_part[blocks] on the way (lb_check reads that one record).
int macro_check_pass(lb_sim *s, bool store)
{
    const dim3 grid((unsigned)((s->pitch / 4 + 255) / 256), (unsigned)s->H);
    const long long blocks = (long long)grid.x * grid.y;
    if (s->check_cap < blocks + 1) {
        if (s->check_part) HIP_TRY(hipFree(s->check_part));
        s->check_part = nullptr;
        s->check_cap = 0;
        HIP_TRY(hipMalloc(&s->check_part, sizeof(CheckPartial) * (size_t)(blocks + 1)));
        s->check_cap = blocks + 1;
        s->bytes += (int64_t)sizeof(CheckPartial) * (blocks + 1);
    }
    if (store)
        hipLaunchKernelGGL(k_macro_check<true>, grid, dim3(256), 0, s->stream, (const float *)s->origin(s->cur), s->plane,
                           (int)s->rowp, (int)s->pitch, s->p.nx, s->rho, s->u, s->v, s->check_part);
    else
        hipLaunchKernelGGL(k_macro_check<false>, grid, dim3(256), 0, s->stream, (const float *)s->origin(s->cur), s->plane,
                           (int)s->rowp, (int)s->pitch, s->p.nx, s->rho, s->u, s->v, s->check_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_check_final, dim3(1), dim3(1024), 0, s->stream, (const CheckPartial *)s->check_part, blocks,
                       s->check_part + blocks);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

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
    int rc = macro_check_pass(s, true);
    if (rc) return rc;
    s->macro_valid = true;
    return LB_OK;
}

// A whole lattice copied on the device by a kernel on the handle's stream (k_copy4: it runs at the streaming ceiling, and it
// is ordered like every other kernel of that stream; hipMemcpyAsync device-to-device goes through the runtime's copy path,
// whose completion the stream did not always wait for when several processes shared the GPU: tools/slab_stress.py).
int copy_lattice(lb_sim *s, float *dst, const float *src)
{
    const long long n4 = s->lat_floats / 4;              // (lat_floats is a multiple of 64)
    hipLaunchKernelGGL(k_copy4<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s->stream,
                       reinterpret_cast<const f4a *>(src), reinterpret_cast<f4a *>(dst), n4);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

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
int lattice_plane_h2d(lb_sim *s, float *origin, int k, const float *host)
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
int lattice_plane_d2h(lb_sim *s, float *host, const float *origin, int k)
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

// Halo of a slab edge, D rows deep: contiguous nx-float row segments ("plane-rows") of the D rows next
// to the edge -- everything a chain of D fused time steps needs to recompute the neighbour's edge rows
// on the way: of the farthest row only the three links that point toward the receiver, of the next one
// those plus its cy=0 links, of the others all nine.
//   D = 3 (18 segments): one three-step launch per exchange; also the format of lb_halo_export/import.
//   D = 6 (45 segments): two three-step launches per exchange (lb_run's six-step cycle);
//   D = 8 (63 segments): two four-step launches per exchange (eight-step cycle).
//   D = 10 (81 segments): two five-step launches per exchange (ten-step cycle, k_step5).
//   D = 12 (99), 14 (117 segments): two six- / seven-step launches per exchange (k_deep).
// "neg" tables hold rows -D..-1 (what leaves through a north edge, counted from row H; what a south
// ghost zone receives, counted from row 0), "pos" tables rows 0..D-1 (leaves south / received north).
// Entry i of an OUT table of one slab pairs with entry i of the IN table of its neighbour.
struct HaloSeg { int k, row; };
constexpr int HALO_SEGS = 18;          // D = 3
constexpr int HALO_SEGS_DEEP = 117;    // D = 14 (99 for D = 12, 81 for D = 10, 63 for D = 8, 45 for D = 6)

struct HaloTables {
    HaloSeg neg[HALO_SEGS_DEEP], pos[HALO_SEGS_DEEP];
    int n = 0;
    explicit HaloTables(int depth)
    {
        static const int up[3] = {2, 5, 6}, down[3] = {4, 7, 8}, flat[3] = {0, 1, 3};
        int i = 0;
        for (int r = -depth; r < 0; ++r) {          // toward the receiver = upward (cy = +1)
            if (r == -depth) { for (int k : up) neg[i++] = {k, r}; }
            else if (r == -depth + 1) { for (int k : flat) neg[i++] = {k, r}; for (int k : up) neg[i++] = {k, r}; }
            else for (int k = 0; k < 9; ++k) neg[i++] = {k, r};
        }
        n = i;
        i = 0;
        for (int r = 0; r < depth; ++r) {           // toward the receiver = downward (cy = -1)
            if (r == depth - 1) { for (int k : down) pos[i++] = {k, r}; }
            else if (r == depth - 2) { for (int k : flat) pos[i++] = {k, r}; for (int k : down) pos[i++] = {k, r}; }
            else for (int k = 0; k < 9; ++k) pos[i++] = {k, r};
        }
    }
    // the same for the pack / unpack kernels (passed by value)
    HaloTable device(bool negative) const
    {
        HaloTable t;
        t.n = n;
        for (int i = 0; i < n; ++i) {
            t.k[i] = (signed char)(negative ? neg[i].k : pos[i].k);
            t.row[i] = (signed char)(negative ? neg[i].row : pos[i].row);
        }
        return t;
    }
};
const HaloTables HALO3(3), HALO6(6), HALO8(8), HALO10(10), HALO12(12), HALO14(14);
const HaloSeg *const NORTH_OUT = HALO3.neg;   // + H
const HaloSeg *const SOUTH_IN = HALO3.neg;    // + 0
const HaloSeg *const SOUTH_OUT = HALO3.pos;   // + 0
const HaloSeg *const NORTH_IN = HALO3.pos;    // + H

float *halo_ptr(const lb_sim *s, int which, const HaloSeg &h, bool north)
{
    const long long row = (north ? s->H : 0) + h.row;
    return s->origin(which) + h.k * s->plane + row * s->rowp;
}

// Pack both edges of lattice `which` into the send buffers / scatter the receive buffers into its
// ghost rows, on stream q.
int halo_pack(lb_sim *s, int which, hipStream_t q, const HaloTables &T, bool to_north, bool to_south)
{
    const size_t n = (size_t)T.n * s->p.nx;
    const bool vec = (s->p.nx % 4) == 0;
    const dim3 grid((s->p.nx + (vec ? 1023 : 255)) / (vec ? 1024 : 256), T.n, 2);
    float *bn = to_north ? s->halo_buf : nullptr, *bs = to_south ? s->halo_buf + n : nullptr;
    if (vec)
        hipLaunchKernelGGL(k_halo_pack<4>, grid, dim3(256), 0, q, (const float *)s->origin(which), s->plane, (int)s->rowp,
                           s->H, s->p.nx, bn, bs, T.device(true), T.device(false));
    else
        hipLaunchKernelGGL(k_halo_pack<1>, grid, dim3(256), 0, q, (const float *)s->origin(which), s->plane, (int)s->rowp,
                           s->H, s->p.nx, bn, bs, T.device(true), T.device(false));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}
int halo_unpack(lb_sim *s, int which, hipStream_t q, const HaloTables &T, const float *from_south, const float *from_north)
{
    const bool vec = (s->p.nx % 4) == 0;
    const dim3 grid((s->p.nx + (vec ? 1023 : 255)) / (vec ? 1024 : 256), T.n, 2);
    if (vec)
        hipLaunchKernelGGL(k_halo_unpack<4>, grid, dim3(256), 0, q, s->origin(which), s->plane, (int)s->rowp, s->H, s->p.nx,
                           from_south, from_north, T.device(true), T.device(false));
    else
        hipLaunchKernelGGL(k_halo_unpack<1>, grid, dim3(256), 0, q, s->origin(which), s->plane, (int)s->rowp, s->H, s->p.nx,
                           from_south, from_north, T.device(true), T.device(false));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int exchange_rccl(lb_sim *s, int which, hipStream_t q, const HaloTables &T)
{
    // neighbours: south = rank-1, north = rank+1; PERIODIC wraps, walls have none
    const bool wrap = (s->p.bc_mode == LB_BC_PERIODIC);
    const int south = (s->rank > 0) ? s->rank - 1 : (wrap ? s->nranks - 1 : -1);
    const int north = (s->rank < s->nranks - 1) ? s->rank + 1 : (wrap ? 0 : -1);
    const size_t n = (size_t)T.n * s->p.nx;
    float *send_n = s->halo_buf, *send_s = s->halo_buf + n, *recv_s = s->halo_buf + 2 * n, *recv_n = s->halo_buf + 3 * n;
    int rc = halo_pack(s, which, q, T, north >= 0, south >= 0);
    if (rc) return rc;
    // One send and one receive per neighbour.  Posting order matters when both neighbours are the same
    // rank (2 ranks, or 1 rank talking to itself, in a periodic box): sends go north-then-south,
    // receives south-then-north, so the n-th send to a peer meets the n-th receive it posted for us.
    NCCL_TRY(g_rccl.GroupStart());
    if (north >= 0) NCCL_TRY(g_rccl.Send(send_n, n, ncclFloat, north, s->comm, q));
    if (south >= 0) NCCL_TRY(g_rccl.Send(send_s, n, ncclFloat, south, s->comm, q));
    if (south >= 0) NCCL_TRY(g_rccl.Recv(recv_s, n, ncclFloat, south, s->comm, q));
    if (north >= 0) NCCL_TRY(g_rccl.Recv(recv_n, n, ncclFloat, north, s->comm, q));
    NCCL_TRY(g_rccl.GroupEnd());
    return halo_unpack(s, which, q, T, south >= 0 ? recv_s : nullptr, north >= 0 ? recv_n : nullptr);
}

// The same exchange over the peer transport: announce, store my edge rows straight into the neighbours' ghost rows, publish
// (kernels_phases.h: k_peer_pre, k_halo_push, k_peer_post), all on stream q.
int exchange_peer(lb_sim *s, int which, hipStream_t q, const HaloTables &T)
{
    PeerArgs pa;
    pa.mine = s->peer_flags;
    pa.south = s->peer_nb[0].flags;
    pa.north = s->peer_nb[1].flags;
    pa.timeout_ticks = s->peer_timeout_ticks;
    pa.which = which;
    hipLaunchKernelGGL(k_peer_pre, dim3(1), dim3(64), 0, q, pa);
    HIP_TRY(hipGetLastError());
    PeerDst dst[2];
    for (int side = 0; side < 2; ++side) {
        const lb_sim::PeerNb &nb = s->peer_nb[side];
        for (int w = 0; w < 2; ++w)
            dst[side].lat[w] = nb.flags ? nb.lat_raw[w] + GUARD + GHOST * nb.rowp : nullptr;
        dst[side].plane = nb.plane; dst[side].rowp = nb.rowp; dst[side].h = nb.h;
    }
    const bool vec = (s->p.nx % 4) == 0;
    const dim3 grid((s->p.nx + (vec ? 1023 : 255)) / (vec ? 1024 : 256), T.n, 2);
    if (vec)
        hipLaunchKernelGGL(k_halo_push<4>, grid, dim3(256), 0, q, (const float *)s->origin(which), s->plane, (int)s->rowp, s->H,
                           s->p.nx, (const unsigned long long *)s->peer_flags, dst[1], dst[0], T.device(true), T.device(false));
    else
        hipLaunchKernelGGL(k_halo_push<1>, grid, dim3(256), 0, q, (const float *)s->origin(which), s->plane, (int)s->rowp, s->H,
                           s->p.nx, (const unsigned long long *)s->peer_flags, dst[1], dst[0], T.device(true), T.device(false));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_peer_post, dim3(1), dim3(64), 0, q, pa);
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

// halo of lattice `which` to the neighbours, by the transport this handle is attached to
int exchange_halo(lb_sim *s, int which, hipStream_t q, const HaloTables &T)
{
    // (lb_exchange_timing: what an exchange takes on its stream -- pack / push, the transfer, the wait for the neighbours, unpack)
    // (not inside a stream capture: timing events cannot be recorded into a graph)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s->xt_on) (void)hipStreamIsCapturing(q, &cap);
    const bool timed = s->xt_on && cap == hipStreamCaptureStatusNone && s->xt_count < lb_sim::XT_RING;
    if (s->xt_on && !timed) ++s->xt_dropped;
    if (timed) HIP_TRY(hipEventRecord(s->xt_ev[2 * s->xt_count], q));
    const int rc = s->peer_connected ? exchange_peer(s, which, q, T) : exchange_rccl(s, which, q, T);
    if (timed && !rc) {
        HIP_TRY(hipEventRecord(s->xt_ev[2 * s->xt_count + 1], q));
        ++s->xt_count;
    }
    return rc;
}

// a wait of the peer transport gave up (the neighbour never arrived): reported once the device is idle
int peer_check_error(lb_sim *s)
{
    if (!s->peer_connected) return LB_OK;
    unsigned long long err = 0;
    HIP_TRY(hipMemcpy(&err, s->peer_flags + PEER_ERR, sizeof(err), hipMemcpyDeviceToHost));
    if (err)
        return fail(LB_ERR_COMM, "peer transport: a neighbour did not arrive at halo exchange %llu within the timeout "
                                 "(LB_PEER_TIMEOUT_S); the state of this handle is not valid", err);
    return LB_OK;
}

// adv (1, 2 or 3) time steps of a slab, edge rows first.  Enqueues on the edge stream (the three
// rows at each end that the halo is cut from) and on the compute stream (the rest), records ev_boundary
// when the edge rows of the new lattice are complete and ev_interior when the interior is.  The caller
// then moves the halo of lattice cur^1 and makes both streams wait for it before the next step.
int slab_step_launch(lb_sim *s, int adv, bool macro)
{
    int rc;
    const int H = s->H;
    macro = macro && !lazy_macro(s);
    if (adv >= 2) {
        const int strips = (s->p.nx + STRIP_W - 1) / STRIP_W;
        const bool three = (adv == 3);
        // edge bands: output rows [0,3) and [H-3,H), one wave per strip and band
        if ((rc = launch_step2(s, s->edge_stream, 0, H, macro, 2, 3, H - 3, 0, three ? 3 : 2))) return rc;
        HIP_TRY(hipEventRecord(s->ev_boundary, s->edge_stream));
        if ((rc = launch_step2(s, s->stream, 3, H - 3, macro, 0, 0, 0, 2 * strips, three ? 3 : 2))) return rc;
    } else {
        // single step: the six rows the 3-deep halo is cut from (0..2, H-3..H-1) first, then the rest
        const hipStream_t keep = s->stream;
        s->stream = s->edge_stream;
        rc = launch_step(s, 0, H - 1, 2, macro);                 // rows 0 and H-1
        if (!rc) rc = launch_step(s, 1, H - 3, 2, macro);        // rows 1 and H-2
        if (!rc) rc = launch_step(s, 2, H - 5, 2, macro);        // rows 2 and H-3
        s->stream = keep;
        if (rc) return rc;
        HIP_TRY(hipEventRecord(s->ev_boundary, s->edge_stream));
        if ((rc = launch_step(s, 3, 1, H - 6, macro))) return rc;
    }
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));
    return LB_OK;
}

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
void launch_costs(const lb_sim *s, float (&cost)[MAX_DEPTH + 1])
{
    static const float seed[MAX_DEPTH + 1] = {0.f, 0.79f, 0.85f, 0.89f, 0.86f, 0.96f, 1.00f, 1.08f};
    double num = 0., den = 0.;
    for (int d = 1; d <= MAX_DEPTH; ++d)
        if (s && s->depth_cost[d] > 0.f) { num += s->depth_cost[d]; den += seed[d]; }
    const float scale = den > 0. ? (float)(num / den) : 1.f;
    cost[0] = 0.f;
    for (int d = 1; d <= MAX_DEPTH; ++d) cost[d] = (s && s->depth_cost[d] > 0.f) ? s->depth_cost[d] : seed[d] * scale;
}
int next_advance(const lb_sim *s, int allowed, int left)
{
    float cost[MAX_DEPTH + 1];
    launch_costs(s, cost);
    return next_advance(allowed, left, cost);
}
int depth_mask(bool two, bool three, bool four = false, bool five = false, bool six = false, bool seven = false)
{
    return 2 | (two ? 4 : 0) | (three ? 8 : 0) | (four ? 16 : 0) | (five ? 32 : 0) | (six ? 64 : 0) | (seven ? 128 : 0);
}

// Both compute streams wait for the other one's kernel and for the halo of the lattice just written.
int slab_step_join(lb_sim *s)
{
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_halo, 0));
    HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_interior, 0));
    HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_halo, 0));
    return LB_OK;
}

// ---- halo cycle of a slab ---------------------------------------------------------------------------
// Two D-step launches per halo exchange, ghost zone 2D rows deep (D = 3 shown; D = 4 likewise with rows
// -8..8); lattice A = cur at the start:
//   edge stream     E1: A rows [-6,6) and [H-6,H+6)  ->  B rows [-3,3) and [H-3,H+3)   (3 ghost rows recomputed)
//   compute stream  C1: A rows [0,H)                 ->  B rows [3,H-3)
//   edge stream     E2: B rows [-3,9) and [H-9,H+3)  ->  A rows [0,6) and [H-6,H)      waits for C1
//   compute stream  C2: B rows [3,H-3)               ->  A rows [6,H-6)                waits for nothing
//   edge stream     pack A's six edge rows -> send/recv -> unpack into A's ghost rows
// and the next C1 waits for E2.  One cross-queue wait per queue and six steps (each costs the waiting
// queue ~6 us, profiles/r01_slab_timeline.txt), and the exchange has until the middle of the NEXT
// cycle to arrive instead of the end of the current launch.
// depth of the fused kernel the halo cycle of a slab runs on: 4 (eight-step cycle), 3 (six-step cycle) or 0
// (no cycle: exchange after every launch).  h = the smallest slab height of the run.
int cycle_depth(const lb_sim *s, int h)
{
    const int v = effective_variant(s);
    if (!(v & VAR_STEP3) || (v & VAR_NO_CYCLE) || !step3_applicable(s, h) || h < 32) return 0;
    // (lb_set_slab_cycle: the caller's choice -- the ranks of a run time the candidates together and agree, bench.py / slabs.py --
    //  wherever that depth can run; elsewhere the automatic one)
    if (s->forced_cycle >= 3 && s->forced_cycle <= MAX_DEPTH && h >= 16 * s->forced_cycle &&
        !(s->forced_cycle >= 6 && s->p.bc_mode == LB_BC_VELOCITY_INLET))
        return s->forced_cycle;
    // (k_deep on slabs, round 5: the fourteen- / twelve-step cycle, ghost zone as deep)
    if ((v & VAR_STEP7) && (v & VAR_STEP6) && (v & VAR_STEP5) && (v & VAR_STEP4) && h >= 112) return 7;
    if ((v & VAR_STEP6) && (v & VAR_STEP5) && (v & VAR_STEP4) && h >= 96) return 6;
    // (k_step5 on slabs: the ten-step cycle, ghost zone ten rows deep)
    if ((v & VAR_STEP5) && (v & VAR_STEP4) && h >= 80) return 5;
    return ((v & VAR_STEP4) && h >= 64) ? 4 : 3;
}
const HaloTables &cycle_halo(int depth)
{
    return depth == 7 ? HALO14 : (depth == 6 ? HALO12 : (depth == 5 ? HALO10 : (depth == 4 ? HALO8 : HALO6)));
}

// bands of output rows [lo_s, hi_s) and [lo_n, hi_n): one wave per strip and band
int launch_bands(lb_sim *s, hipStream_t st, int lo_s, int hi_s, int lo_n, int hi_n, bool macro, int depth)
{
    if (hi_s - lo_s == hi_n - lo_n)
        return launch_step2(s, st, lo_s, hi_n, macro, 2, hi_s - lo_s, lo_n - lo_s, 0, depth);
    int rc = launch_step2(s, st, lo_s, hi_s, macro, 1, hi_s - lo_s, 0, 0, depth);
    if (!rc) rc = launch_step2(s, st, lo_n, hi_n, macro, 1, hi_n - lo_n, 0, 0, depth);
    return rc;
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
int band_extra(const lb_sim *s, int D, bool split = false)
{
    if (D < 4) return 0;                                // (k_step2 / k_step3: one wave per strip and band, a few rows: as they were)
    // (one launch per band: the exchange must fit into the head start; split: only the launch gaps of the two parts do)
    const double slack = split ? 3.0 : 8.0;
    const int H = s->H;
    const int room = (H - 4 * D) / 2 - 8;               // the interior of the second launch keeps at least 16 rows
    if (room <= 0) return 0;
    const int strips = D >= 6 ? deep_strips(s->p.nx, D) : (D == 5 ? step5_strips(s->p.nx) : (s->p.nx + STRIP_W - 1) / STRIP_W);
    const int wpc = D >= 6 ? 4 : 8;
    const int segs = std::max(1, (s->cu_count * wpc - 2 * strips * STEP4_WAVES) / STEP4_WAVES / strips);    // interior pairs per strip
    const double cost = s->p.bc_mode == LB_BC_PERIODIC ? 1.0 : (D >= 6 ? 2.1 : 1.2);    // a wall-column strip's rows (launch_step2)
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

// E1 + C1 (the caller flips cur afterwards); D = depth of the fused kernel (3 or 4).  last = this launch ends the run:
// rho,u,v are stored and the ghost rows are not recomputed (nothing will consume them; the MACRO epilogue has no rows
// outside the slab to write to).  split: the bands in two launches, the outer one behind the exchange on the communication
// stream (ev_halo); else the caller has put the exchange on the edge stream itself.
int slab_cycle_first(lb_sim *s, int D, bool last = false, bool split = false)
{
    const int H = s->H, strips = D >= 6 ? deep_strips(s->p.nx, D) : (D == 5 ? step5_strips(s->p.nx) : (s->p.nx + STRIP_W - 1) / STRIP_W);
    const StepArgs probe = step_args(s, 0, 1, 1);
    const bool macro = last && !lazy_macro(s);
    const int B = band_extra(s, D, split);
    const int lo = (probe.ghost_s && !last) ? -D : 0, hi = (probe.ghost_n && !last) ? H + D : H;
    int rc;
    if (split && B > 0) {
        if ((rc = launch_bands(s, s->edge_stream, D, D + B, H - D - B, H - D, macro, D))) return rc;      // E1b
        HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_halo, 0));
        if ((rc = launch_bands(s, s->edge_stream, lo, D, H - D, hi, macro, D))) return rc;                 // E1a
    } else {
        if (split) HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_halo, 0));
        if ((rc = launch_bands(s, s->edge_stream, lo, D + B, H - D - B, hi, macro, D))) return rc;
    }
    // (wave slots left to the band launch running beside it: two bands x strips items, two waves each under k_step4)
    if ((rc = launch_step2(s, s->stream, D + B, H - D - B, macro, 0, 0, 0, 2 * strips * (D >= 4 ? STEP4_WAVES : 1), D))) return rc;
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));
    return LB_OK;
}

// E2 + C2 (the caller flips cur afterwards); ev_edge = the 2D edge rows of the new lattice are complete (the exchange may start),
// ev_boundary = all of the bands' rows are (the next C1 may)
int slab_cycle_second(lb_sim *s, bool macro, int D, bool split = false)
{
    const int H = s->H, strips = D >= 6 ? deep_strips(s->p.nx, D) : (D == 5 ? step5_strips(s->p.nx) : (s->p.nx + STRIP_W - 1) / STRIP_W);
    macro = macro && !lazy_macro(s);
    const int B = band_extra(s, D, split);
    HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_interior, 0));
    int rc;
    if (split && B > 0) {
        if ((rc = launch_bands(s, s->edge_stream, 0, 2 * D, H - 2 * D, H, macro, D))) return rc;                              // E2a
        HIP_TRY(hipEventRecord(s->ev_edge, s->edge_stream));
        if ((rc = launch_bands(s, s->edge_stream, 2 * D, 2 * D + B, H - 2 * D - B, H - 2 * D, macro, D))) return rc;          // E2b
    } else {
        if ((rc = launch_bands(s, s->edge_stream, 0, 2 * D + B, H - 2 * D - B, H, macro, D))) return rc;
        HIP_TRY(hipEventRecord(s->ev_edge, s->edge_stream));
    }
    HIP_TRY(hipEventRecord(s->ev_boundary, s->edge_stream));
    return launch_step2(s, s->stream, 2 * D + B, H - 2 * D - B, macro, 0, 0, 0, 2 * strips * (D >= 4 ? STEP4_WAVES : 1), D);
}

// Which fused depths a whole-grid handle may use: the variant bits (explicit or from the size heuristic), or --
// once lb_autotune has timed this grid -- everything applicable up to the depth it found fastest.
// Four steps per pass through LDS tiles (k_tile4) instead of the marching kernels: asked for (VAR_TILES),
// found fastest by lb_autotune, or -- automatic -- on whole grids below ~1400^2 cells and on grids the marching
// kernels do not serve (27 k MLUPS at 256^2, 82 k at 512^2, 120 k at 1024^2, 138 k at 1280^2, against 19 / 57 /
// 113 / 129 k; from 1536^2 the marching kernel wins, 163 against 153 k: profiles/r01_sweep_variants.txt).
bool use_tile_kernel(const lb_sim *s)
{
    if (!tile_applicable(s)) return false;
    if (s->variant >= 0) return (s->variant & VAR_TILES) != 0;
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

int whole_grid_depths(const lb_sim *s)
{
    if (use_tile_kernel(s)) return depth_mask(false, false, true);      // k_tile4 + single steps for the remainder
    if (s->variant < 0 && s->tuned_steps)
        return depth_mask(step2_applicable(s) && s->tuned_steps >= 2, step3_applicable(s) && s->tuned_steps >= 3,
                          step4_applicable(s) && s->tuned_steps >= 4, step5_applicable(s) && s->tuned_steps >= 5,
                          deep_applicable(s) && s->tuned_steps >= 6, deep_applicable(s) && s->tuned_steps >= 7);
    const int v = effective_variant(s);
    return depth_mask((v & VAR_STEP2) && step2_applicable(s), (v & VAR_STEP3) && step3_applicable(s), (v & VAR_STEP4) && step4_applicable(s),
                      (v & VAR_STEP5) && step5_applicable(s), (v & VAR_STEP6) && deep_applicable(s), (v & VAR_STEP7) && deep_applicable(s));
}

// A d-step pass (d = 3, 4, 5) of the velocity-inlet family.  Rows [d, ny-d) depend on nothing the wall rows do within d steps:
// the marching kernel takes them, treating the wall rows as don't-care like any wall.  The 2d wall-side rows are advanced
// as a lattice of their own: the 2d rows next to each wall, stacked, ARE a velocity-inlet lattice of 4d rows -- row 0's pull
// reaches "row ny-2" = band row 4d-2, row ny-1's "row 1" = band row 1 -- except at the seam in the middle, whose garbage
// travels one row per step and after d steps has reached exactly the rows that are not needed.  One launch (k_vel_band:
// column chunks of the band in LDS, d steps there, the outer d + d rows stored) on the edge stream beside the interior's:
// both only read the current lattice and write disjoint rows of the other one.  (Round 2: the bands were copied into a
// second handle, stepped d times there and copied back -- a chain of a dozen small launches.)
int vel_band_pass(lb_sim *s, int d, bool macro)
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
    if ((rc = launch_step2(s, s->stream, d, H - d, macro, 0, 0, 0, 0, d))) return rc;
    HIP_TRY(hipEventRecord(s->ev_boundary, q));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));   // the next pass (or the caller) sees the bands in place
    return LB_OK;
}

// n time steps on a whole-grid handle: largest fused kernel first in the remainder (n = 3a + rem with
// the three-step kernel, 2a + rem with the two-step kernel), hipGraph replay for small grids.
int run_whole_grid(lb_sim *s, int n_steps, bool final_macro = true)
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
        else if (adv >= 2) rc = launch_step2(s, s->stream, 0, s->H, macro, 0, 0, 0, 0, adv);
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

// Time the candidate configurations of the fused kernels on LIVE steps (every configuration produces
// bitwise identical results, so tuning advances the simulation like any other steps): four-, three- and
// two-step marching kernels at 8 and 4 waves per CU, and the single-step kernel.  Which one wins depends
// on the grid's aspect ratio, the mask and the boundary family (wide, short pipes favour fewer, longer
// segments: +20 % at 3751 x 1251).  Returns the number of steps advanced, or a negative status.  max_steps: the caller's budget --
// the rounds are the caller's to fit into it (autotune_quick_cost), the runner-up pass below is skipped where it would not fit.
void tune_cache_store(const lb_sim *s);                 // (LB_TUNE_CACHE, below)

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

// VELOCITY_INLET: where the eight never-written corner links live in a lattice (bc_vel_cell's order): {link, x, y}
struct CornerLink { int k, x, y; };
void corner_links(const lb_sim *s, CornerLink (&c)[8])
{
    const int X = s->p.nx - 1, Y = s->p.ny - 1;
    const CornerLink t[8] = {{1, 0, 0}, {8, 0, 0}, {1, 0, Y}, {5, 0, Y}, {3, X, 0}, {7, X, 0}, {3, X, Y}, {6, X, Y}};
    for (int i = 0; i < 8; ++i) c[i] = t[i];
}
// ... copied out of lattice `which` whenever the populations are set as a whole (the reference's f_streamed = f at
// that moment, opencl_dim.py:323-327), and written back into it before the un-fused boundary phase reads them
int corners_capture(lb_sim *s, int which)
{
    if (s->p.bc_mode != LB_BC_VELOCITY_INLET) return LB_OK;
    CornerLink c[8];
    corner_links(s, c);
    for (int i = 0; i < 8; ++i)
        HIP_TRY(hipMemcpyAsync(s->vi_corner + i, s->origin(which) + c[i].k * s->plane + (long long)c[i].y * s->rowp + c[i].x,
                               sizeof(float), hipMemcpyDeviceToDevice, s->stream));
    return LB_OK;
}
int corners_patch(lb_sim *s, int which)
{
    CornerLink c[8];
    corner_links(s, c);
    for (int i = 0; i < 8; ++i)
        HIP_TRY(hipMemcpyAsync(s->origin(which) + c[i].k * s->plane + (long long)c[i].y * s->rowp + c[i].x, s->vi_corner + i,
                               sizeof(float), hipMemcpyDeviceToDevice, s->stream));
    return LB_OK;
}

// steps a quick (one-round) tuning pass consumes at most: 11 candidates x 2 samples x 12 (36) steps, 2 x 2 x 10, 2 x 2 x 14, + 1
// (an upper bound: every candidate usable).  The runner-up pass of autotune_whole_grid is not counted: it only runs where the
// budget it is given holds it, and lb_autotune_quick gives it max_steps, so the quick pass never advances more than max_steps.
int autotune_quick_cost(const lb_sim *s) { return 11 * 2 * (small_grid(s) ? 36 : 12) + 2 * 2 * 10 + 2 * 2 * 14 + 1; }

// the Cython path runs four steps per launch through LDS tiles (k1_tile4) unless the grid is too small for them or an
// explicit variant without VAR_TILES asks for single steps (k1_fstep)
bool cython_tiles(const lb_sim *s) { return s->p.nx >= 64 && s->H >= 64 && (s->variant < 0 || (s->variant & VAR_TILES)); }

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

bool tune_entry_runs_here(const lb_sim *s, const TuneEntry &e);

// takes over a remembered result; true if the handle is tuned afterwards
bool tune_cache_apply(lb_sim *s)
{
    s->tune_cache_checked = true;
    const char *path = tune_cache_path();
    if (!path || s->variant >= 0 || s->tuned_steps) return s->tuned_steps != 0;
    std::lock_guard<std::mutex> lock(g_tune_mu);
    tune_cache_load_locked(path);
    auto it = g_tune.find(tune_key(s));
    if (it == g_tune.end() || !tune_entry_runs_here(s, it->second)) return false;
    s->tuned_steps = it->second.steps;
    s->tuned_wpc = it->second.wpc;
    for (int d = 0; d <= MAX_DEPTH; ++d) s->depth_cost[d] = d ? it->second.cost[d] : 0.f;
    return true;
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

bool autotune_applies(const lb_sim *s)
{
    return !s->multi_slab() && s->p.semantics != LB_SEM_CYTHON &&
           (step2_applicable(s) || step3_applicable(s) || tile_applicable(s));
}

bool tune_entry_runs_here(const lb_sim *s, const TuneEntry &e)
{
    if (!autotune_applies(s) || e.steps < 1 || e.steps > MAX_DEPTH) return false;
    if (e.steps >= 6) return deep_applicable(s) && (e.wpc == 4 || (e.steps == 7 && e.wpc == 8));
    if (e.steps == 5) return step5_applicable(s) && (e.wpc == 8 || e.wpc == 6);
    if (e.steps == 4) return e.wpc < 0 ? tile_applicable(s) : (step4_applicable(s) && (e.wpc == 8 || e.wpc == 6 || e.wpc == 4));
    if (e.steps == 3) return step3_applicable(s) && (e.wpc == 8 || e.wpc == 6 || e.wpc == 4);
    if (e.steps == 2) return step2_applicable(s) && (e.wpc == 8 || e.wpc == 4);
    return e.wpc == 0;
}

}  // namespace

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
    if (p->bc_mode < LB_BC_PIPE || p->bc_mode > LB_BC_VELOCITY_INLET) return fail(LB_ERR_ARG, "unknown bc_mode %d", p->bc_mode);
    if (p->bc_mode == LB_BC_VELOCITY_INLET &&
        (p->local_ny != p->ny || (p->flags & LB_FLAG_HALO) || p->semantics != LB_SEM_OPENCL))
        return fail(LB_ERR_ARG, "the velocity-inlet family exists for whole-grid OpenCL-path handles only");
    if (p->bc_mode == LB_BC_VELOCITY_INLET && (!(p->inlet_u < 1.f) || !(p->outlet_u > -1.f)))
        return fail(LB_ERR_ARG, "velocity-inlet speeds must satisfy inlet_u < 1 and outlet_u > -1");
    if (!(p->omega > 0.f && p->omega < 2.f)) return fail(LB_ERR_ARG, "omega must be in (0,2), got %g", p->omega);
    for (int r : p->reserved)
        if (r != 0) return fail(LB_ERR_ARG, "reserved fields must be zero");
    if (p->flags & ~(LB_FLAG_HALO | LB_FLAG_PLANAR | LB_FLAG_EAGER_MACRO)) return fail(LB_ERR_ARG, "unknown flags 0x%x", p->flags);
    if (p->semantics != LB_SEM_OPENCL && p->semantics != LB_SEM_CYTHON && p->semantics != LB_SEM_OPENCL_D2Q9I)
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

#define CREATE_TRY(expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fail(LB_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));                   \
            lb_destroy(s);                                                                     \
            return LB_ERR_HIP;                                                                 \
        }                                                                                      \
    } while (0)
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
    CREATE_TRY(hipMalloc(&s->vi_corner, 8 * sizeof(float)));
    CREATE_TRY(hipMemsetAsync(s->vi_corner, 0, 8 * sizeof(float), s->stream));
    CREATE_TRY(hipMalloc(&s->mask_raw, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD));
    s->mask = s->mask_raw + GUARD + MASK_GHOST * s->pitch;
    CREATE_TRY(hipMemsetAsync(s->rho, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->u, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->v, 0, fld_bytes, s->stream));
    CREATE_TRY(hipMemsetAsync(s->mask_raw, 0, (size_t)s->pitch * (s->H + 2 * MASK_GHOST) + 2 * GUARD, s->stream));
    CREATE_TRY(hipStreamSynchronize(s->stream));
#undef CREATE_TRY
    s->bytes = 2 * lat_bytes + 3 * fld_bytes + (size_t)s->pitch * s->H;
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
    for (float *p : {s->lat[0], s->lat[1], s->feq, s->rho, s->u, s->v, s->halo_buf, s->vi_corner, s->stage})
        if (p) (void)hipFree(p);
    if (s->mask_raw) (void)hipFree(s->mask_raw);
    if (s->check_part) (void)hipFree(s->check_part);
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
    s->variant = variant;
    return LB_OK;
}

int lb_set_slab_cycle(lb_sim *s, int depth)
{
    if (s && s->cpu) return LB_OK;
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
    if (!s) return fail(LB_ERR_ARG, "null handle");
    s->xchg_inline = on != 0;
    return LB_OK;
}

int lb_exchange_timing(lb_sim *s, int enable)
{
    CPU_UNSUPPORTED(s, "lb_exchange_timing");
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
    const int D = s->multi_slab() ? cycle_depth(s, s->min_h > 0 ? s->min_h : s->H) : 0;
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
    if ((rc = corners_capture(s, s->cur))) return rc;
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
    if (!s || !out8) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipMemcpyAsync(out8, s->vi_corner, 8 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_set_corner_state(lb_sim *s, const float *in8)
{
    CPU_UNSUPPORTED(s, "lb_set_corner_state");
    if (!s || !in8) return fail(LB_ERR_ARG, "null argument");
    DeviceGuard guard(s->p.device);
    HIP_TRY(hipMemcpyAsync(s->vi_corner, in8, 8 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LB_OK;
}

int lb_update_feq(lb_sim *s);
int lb_steps_per_launch(lb_sim *s);

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
static dim3 cells_grid(const lb_sim *s, int nz) { return dim3((s->p.nx + 255) / 256, s->p.ny, nz); }

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
    // VELOCITY_INLET: the eight corner links no phase ever writes are kept apart (fused launches swap the lattices,
    // so "whatever f_streamed held" would not survive them): put them where the boundary phase reads them
    if (s->p.bc_mode == LB_BC_VELOCITY_INLET) return corners_patch(s, s->cur);
    return LB_OK;
}

int lb_move_bcs(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->move_bcs(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_move_bcs");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    if ((rc = ensure_macro(s))) return rc;
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

int lb_update_hydro(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->update_hydro(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_update_hydro");
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
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
    PhaseArgs a = phase_args(s);
    a.ny = s->H;   // rho,u,v are local: valid for slabs too
    if (s->p.semantics == LB_SEM_OPENCL_D2Q9I)
        hipLaunchKernelGGL(k_feq_i, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    else
        hipLaunchKernelGGL(k_feq, dim3((s->p.nx + 255) / 256, s->H, 1), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    s->feq_valid = true;
    return LB_OK;
}

int lb_collide_particles(lb_sim *s)
{
    if (s && s->cpu) { s->cpu->collide(); return LB_OK; }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int rc = need_single_slab(s, "lb_collide_particles");
    if (rc) return rc;
    if (!s->feq) return fail(LB_ERR_STATE, "lb_collide_particles before any lb_update_feq");
    DeviceGuard guard(s->p.device);
    if ((rc = ensure_macro(s))) return rc;
    hipLaunchKernelGGL(k_collide, cells_grid(s, 9), dim3(256), 0, s->stream, phase_args(s));
    HIP_TRY(hipGetLastError());
    return LB_OK;
}

int lb_zero_velocity_in_obstacle(lb_sim *s)
{
    if (s && s->cpu) {
        for (size_t c = 0; s->cpu->has_mask && c < s->cpu->plane(); ++c)
            if (s->cpu->mask[c]) { s->cpu->u[c] = 0.; s->cpu->v[c] = 0.; }
        return LB_OK;
    }
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
    return corners_capture(s, s->cur);
}

// ---- fused stepping ----------------------------------------------------------------------
int lb_step_boundary(lb_sim *s, int write_macro)
{
    CPU_UNSUPPORTED(s, "lb_step_boundary");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_step_boundary called twice");
    if (s->p.bc_mode == LB_BC_VELOCITY_INLET || s->p.semantics == LB_SEM_CYTHON)
        return fail(LB_ERR_STATE, "no split step for this boundary family / semantics: use lb_run");
    DeviceGuard guard(s->p.device);
    // local rows 0 and H-1 (one row when H == 1)
    int rc = launch_step(s, 0, s->H > 1 ? s->H - 1 : 1, s->H > 1 ? 2 : 1, write_macro != 0);
    if (rc) return rc;
    s->stepping = 1;
    return LB_OK;
}

int lb_step_interior(lb_sim *s, int write_macro)
{
    CPU_UNSUPPORTED(s, "lb_step_interior");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (!s->stepping) return fail(LB_ERR_STATE, "lb_step_interior before lb_step_boundary");
    DeviceGuard guard(s->p.device);
    return launch_step(s, 1, 1, s->H - 2, write_macro != 0);
}

int lb_step_finish(lb_sim *s)
{
    CPU_UNSUPPORTED(s, "lb_step_finish");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (!s->stepping) return fail(LB_ERR_STATE, "lb_step_finish before lb_step_boundary");
    s->cur ^= 1;
    s->stepping = 0;
    s->feq_valid = false;
    s->macro_valid = !lazy_macro(s);      // (rebuilt on demand there; the other families stored them if write_macro said so)
    s->ghost_depth = 0;   // the caller imports the new ghosts (lb_run manages its own)
    return LB_OK;
}

int lb_halo_export(lb_sim *s, int side, void *buf)
{
    CPU_UNSUPPORTED(s, "lb_halo_export");
    if (!s || !buf || side < 0 || side > 1) return fail(LB_ERR_ARG, "bad argument");
    DeviceGuard guard(s->p.device);
    const int which = s->stepping ? (s->cur ^ 1) : s->cur;
    const HaloSeg *tab = side ? NORTH_OUT : SOUTH_OUT;
    for (int i = 0; i < HALO_SEGS; ++i)
        HIP_TRY(hipMemcpyAsync((float *)buf + (size_t)i * s->p.nx, halo_ptr(s, which, tab[i], side != 0),
                               sizeof(float) * s->p.nx, hipMemcpyDefault, s->stream));
    return LB_OK;
}

int lb_halo_import(lb_sim *s, int side, const void *buf)
{
    CPU_UNSUPPORTED(s, "lb_halo_import");
    if (!s || !buf || side < 0 || side > 1) return fail(LB_ERR_ARG, "bad argument");
    DeviceGuard guard(s->p.device);
    const int which = s->stepping ? (s->cur ^ 1) : s->cur;
    const HaloSeg *tab = side ? NORTH_IN : SOUTH_IN;
    for (int i = 0; i < HALO_SEGS; ++i)
        HIP_TRY(hipMemcpyAsync(halo_ptr(s, which, tab[i], side != 0), (const float *)buf + (size_t)i * s->p.nx,
                               sizeof(float) * s->p.nx, hipMemcpyDefault, s->stream));
    return LB_OK;
}

int lb_halo_floats(lb_sim *s)
{
    CPU_UNSUPPORTED(s, "lb_halo_floats");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    return HALO_SEGS * s->p.nx;
}

namespace {
// one halo cycle of lb_run: E1 + C1, E2 + C2 in split bands, exchange of the 2D edge rows (see slab_cycle_first) on the communication
// stream, behind the outer part of E2 (ev_edge) and in front of the outer part of the next E1 (ev_halo).
int slab_cycle_one(lb_sim *s, int D, bool last_of_run, const HaloTables &T)
{
    int rc;
    if ((rc = slab_cycle_first(s, D, false, true))) return rc;
    s->cur ^= 1;
    if ((rc = slab_cycle_second(s, last_of_run, D, true))) return rc;
    s->cur ^= 1;
    // (xchg_inline: on the compute stream, i.e. behind C2 and in front of the next C1 -- beside the tail of E2b at most)
    hipStream_t xq = s->xchg_inline ? s->stream : s->comm_stream;
    HIP_TRY(hipStreamWaitEvent(xq, s->ev_edge, 0));
    if ((rc = exchange_halo(s, s->cur, xq, T))) return rc;
    HIP_TRY(hipEventRecord(s->ev_halo, xq));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));
    return LB_OK;
}
}  // namespace

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
    if (!s->tune_cache_checked) (void)tune_cache_apply(s);
    int rc;
    if (s->p.semantics == LB_SEM_CYTHON) {
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
        // grids too small for tiles, or LB_VARIANT / lb_set_variant without VAR_TILES with an explicit variant: single steps only
        const dim3 blk(64, 4), grd((unsigned)((s->pitch / 4 + 63) / 64), (unsigned)((s->H + 3) / 4));
        // (rounds 4-5 also had a five-step marching form, k1_step5: bitwise right, slower than the tiles at the reference's sizes --
        //  3751 x 1251 with the cylinder 136 against 174 k MLUPS --, diagnostic build only in round 5, removed in round 6)
        const bool tiles = cython_tiles(s);
        int left = n_steps;
        while (left > 0) {
            const PhaseArgs a = phase_args(s);
            if (tiles && left % TILE_T == 0) {
                const int tiles_x = (s->p.nx + 31) / 32, tiles_y = (s->H + 15) / 16, n_tiles = tiles_x * tiles_y;
                const dim3 tg((n_tiles + 7) / 8 * 8), tb(TileShape<32, 16, 2>::THREADS);    // (eight equal shares: xcd_band_tile)
                const bool lastp = (left == TILE_T);
#define LB_LAUNCH1T(MASK)                                                                                                  \
                do {                                                                                                       \
                    if (lastp) hipLaunchKernelGGL((k1_tile4<MASK, true, false>), tg, tb, 0, s->stream, a, tiles_x, n_tiles); \
                    else hipLaunchKernelGGL((k1_tile4<MASK, false, true>), tg, tb, 0, s->stream, a, tiles_x, n_tiles);       \
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
    if (!s->multi_slab()) return run_whole_grid(s, n_steps);     // (never blocks the host: tuning is lb_autotune*'s job)
    if (!s->comm && !s->peer_connected)
        return fail(LB_ERR_STATE, "lb_run on a slab handle needs lb_comm_init or lb_peer_connect (or drive lb_step_* yourself)");
    if (n_steps == 0) return LB_OK;
    if (s->H < 6) return fail(LB_ERR_ARG, "a slab needs at least 6 rows (has %d)", s->H);
    // Two queues.  The edge stream carries the dependency chain of the slab as it is:
    // edge rows of step t -> pack -> RCCL send/recv -> unpack -> edge rows of step t+1, in order, no
    // events in between.  The compute stream carries the interior rows.  Across the two, per launch:
    // the edge kernel waits for the previous interior kernel (it reads 3 rows past the band), the
    // interior kernel for the previous edge kernel (it reads rows 0..H-1, never the ghost rows, so it
    // does not wait for the exchange).  Every cross-queue wait costs ~2 us per step on this part even
    // when long satisfied (profiles/r01_slab_timeline.txt), hence as few as the data flow allows.
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_interior, 0));
    int left = n_steps;
    const int hmin = s->min_h > 0 ? s->min_h : s->H;     // all ranks decide on the same height
    const int D = cycle_depth(s, hmin);
    if (D && left >= D) {
        // 2D-step cycles (see slab_cycle_first), then -- D <= left < 2D -- one lone first half (D steps out of D-deep
        // ghosts: e.g. 20 steps = two eight-step cycles + one four-step launch); what is left after that (< D steps) runs
        // launch by launch below.  One deep exchange serves both.
        const HaloTables &T = cycle_halo(D);
        // (a first half that is not the run's last launch recomputes D ghost rows of the new lattice on the way and reads 2D
        // deep for that; only the very last launch gets by with D.  With `left >= 2D ? 2D : D` here, run(29) + run(4) on the
        // six-step cycle started the second run's first half from 3-deep ghosts: rows 0 and H-1 wrong one step later --
        // found by tools/ring_stress.py)
        if (s->ghost_depth < (left == D ? D : 2 * D)) {
            if ((rc = exchange_halo(s, s->cur, s->edge_stream, T))) return rc;
            s->ghost_depth = 2 * D;
        }
        // (the exchanges of the cycles below run on the communication stream, each behind the outer edge rows of its cycle and in front
        //  of the next cycle's; whatever the edge stream has done so far -- the exchange above -- precedes the first of them)
        HIP_TRY(hipEventRecord(s->ev_halo, s->edge_stream));
        HIP_TRY(hipStreamWaitEvent(s->xchg_inline ? s->stream : s->comm_stream, s->ev_halo, 0));
        for (; left >= 2 * D; left -= 2 * D) {
            if ((rc = slab_cycle_one(s, D, left == 2 * D, T))) return rc;
            s->ghost_depth = 2 * D;
        }
        if (left >= D) {
            const bool last = (left == D);
            if ((rc = slab_cycle_first(s, D, last, true))) return rc;
            HIP_TRY(hipEventRecord(s->ev_boundary, s->edge_stream));      // the edge bands of the new lattice are complete
            s->cur ^= 1;
            left -= D;
            s->ghost_depth = last ? 0 : D;          // rows [-D,0) and [H,H+D) of the new lattice were recomputed on the way
            HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));
            HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_interior, 0));
        }
        // (whatever follows on the edge stream follows the last exchange of the cycles)
        HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_halo, 0));
    }
    if (left > 0 && s->ghost_depth < 3) {
        // ghost rows of the current lattice: exchange once before the first step
        if ((rc = exchange_halo(s, s->cur, s->edge_stream, HALO3))) return rc;
    }
    const bool two = (effective_variant(s) & VAR_STEP2) && step2_applicable(s, hmin);
    const bool three = (effective_variant(s) & VAR_STEP3) && step3_applicable(s, hmin);
    const bool stepped = left > 0;
    while (left > 0) {
        const int adv = next_advance(s, depth_mask(two, three), left);
        // 1. edge rows (edge stream) and interior rows (compute stream) of the new lattice, concurrently
        if ((rc = slab_step_launch(s, adv, left == adv))) return rc;
        // 2. halo of the lattice just written, behind the edge kernel on its stream (RCCL over xGMI),
        //    while the interior is still being computed
        if ((rc = exchange_halo(s, s->cur ^ 1, s->edge_stream, HALO3))) return rc;
        // 3. the next launches read the new lattice
        HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_boundary, 0));
        HIP_TRY(hipStreamWaitEvent(s->edge_stream, s->ev_interior, 0));
        s->cur ^= 1;
        left -= adv;
    }
    // the caller's stream sees the whole state, ghost rows included
    HIP_TRY(hipEventRecord(s->ev_halo, s->edge_stream));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_halo, 0));
    if (stepped) s->ghost_depth = 3;
    s->feq_valid = false;
    s->macro_valid = !lazy_macro(s);
    return LB_OK;
}

// Virtual slabs: `count` slab handles that together tile one grid (handle i = slab i, south to north),
// all on one device, advanced in lock step with device-to-device halo copies.  Same kernels, same
// schedule and same halo tables as the RCCL path; exists so that the slab code can be verified
// bitwise against the undivided run on a single GPU.
// Full device synchronisation at chosen points of lb_run_group (bits: 1 after every launch phase, 2 after every exchange,
// 4 after every step, 8 at entry and exit); default 0 = the members' streams are ordered by events alone, as lb_run's are.
// History: with the edge streams at the device's highest priority and several processes sharing the GPU, rare partitions
// (1-2 in a hundred) differed from the undivided run in the event-only schedule; round 2 hid that behind a join after every
// exchange (bit 2).  Round 3: the edge stream runs at normal priority (lb_create) and the event-only schedule passes 650 of
// 650 random partitions under the same contention, so the harness checks what lb_run relies on again.  lb_set_debug_sync /
// LB_DEBUG_SYNC remain for diagnosis.
static int g_debug_sync = -1;         // < 0: not read from the environment yet
static int debug_sync_bits()
{
    if (g_debug_sync < 0) g_debug_sync = getenv("LB_DEBUG_SYNC") ? atoi(getenv("LB_DEBUG_SYNC")) & 15 : 0;
    return g_debug_sync;
}
int lb_set_debug_sync(int bits)
{
    const int prev = debug_sync_bits();
    g_debug_sync = bits & 15;
    return prev;
}
#define DBG_SYNC(bit)                                                   \
    do {                                                                \
        if (debug_sync_bits() & (bit)) HIP_TRY(hipDeviceSynchronize()); \
    } while (0)

int lb_run_group(lb_sim **sims, int count, int n_steps)
{
    for (int i = 0; sims && i < count; ++i) CPU_UNSUPPORTED(sims[i], "lb_run_group");
    if (!sims || count < 1 || n_steps < 0) return fail(LB_ERR_ARG, "bad argument");
    for (int i = 0; i < count; ++i) {
        if (!sims[i]) return fail(LB_ERR_ARG, "null handle in group");
        if (!sims[i]->multi_slab()) return fail(LB_ERR_ARG, "group members must be slab handles (LB_FLAG_HALO)");
        if (sims[i]->p.device != sims[0]->p.device) return fail(LB_ERR_ARG, "group members must share a device");
        if (sims[i]->stepping) return fail(LB_ERR_STATE, "lb_run_group inside a split step");
        if (sims[i]->H < 6) return fail(LB_ERR_ARG, "a slab needs at least 6 rows");
    }
    if (n_steps == 0) return LB_OK;
    DeviceGuard guard(sims[0]->p.device);
    DBG_SYNC(8);
    const bool wrap = (sims[0]->p.bc_mode == LB_BC_PERIODIC);
    int rc;
    // halo (3 rows deep) of lattice `rel` (0 = current, 1 = the one being written) of every member: each packs its edge
    // rows into its send buffers on its communication stream once they are complete, the receivers scatter them from
    // there into their ghost rows (the kernels of the RCCL path, with the transport replaced by a plain read of the
    // neighbour's buffer)
    for (int i = 0; i < count; ++i)
        if (!sims[i]->halo_buf) {
            HIP_TRY(hipMalloc(&sims[i]->halo_buf, sizeof(float) * 4 * HALO_SEGS_DEEP * sims[i]->p.nx));
            sims[i]->bytes += sizeof(float) * 4 * HALO_SEGS_DEEP * sims[i]->p.nx;
        }
    auto south_nb = [&](int i) { return i > 0 ? i - 1 : (wrap ? count - 1 : -1); };
    auto north_nb = [&](int i) { return i < count - 1 ? i + 1 : (wrap ? 0 : -1); };
    auto exchange = [&](int rel, bool wait_edges) -> int {
        const size_t n3 = (size_t)HALO3.n * sims[0]->p.nx;
        for (int i = 0; i < count; ++i) {
            lb_sim *me = sims[i];
            // my edge rows are complete; my send buffers are free (both neighbours have read the previous halo out of them)
            HIP_TRY(hipStreamWaitEvent(me->comm_stream, wait_edges ? me->ev_boundary : me->ev_interior, 0));
            for (int nb : {south_nb(i), north_nb(i)})
                if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->comm_stream, sims[nb]->ev_halo, 0));
            if ((rc = halo_pack(me, me->cur ^ rel, me->comm_stream, HALO3, north_nb(i) >= 0, south_nb(i) >= 0))) return rc;
            HIP_TRY(hipEventRecord(me->ev_packed, me->comm_stream));
        }
        for (int i = 0; i < count; ++i) {
            lb_sim *me = sims[i];
            const int so = south_nb(i), no = north_nb(i);
            for (int nb : {so, no})
                if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->comm_stream, sims[nb]->ev_packed, 0));
            // my south ghost rows <- what the southern neighbour sent north, and vice versa
            if ((rc = halo_unpack(me, me->cur ^ rel, me->comm_stream, HALO3, so >= 0 ? sims[so]->halo_buf : nullptr,
                                  no >= 0 ? sims[no]->halo_buf + n3 : nullptr)))
                return rc;
            HIP_TRY(hipEventRecord(me->ev_halo, me->comm_stream));
        }
        return LB_OK;
    };
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipEventRecord(sims[i]->ev_interior, sims[i]->stream));
        HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[i]->ev_interior, 0));
    }
    int hmin = sims[0]->H;
    for (int i = 1; i < count; ++i) hmin = std::min(hmin, sims[i]->H);
    bool two = true, three = true;
    int D = MAX_DEPTH;
    for (int i = 0; i < count; ++i) {
        two = two && (effective_variant(sims[i]) & VAR_STEP2) && step2_applicable(sims[i], hmin);
        three = three && (effective_variant(sims[i]) & VAR_STEP3) && step3_applicable(sims[i], hmin);
        D = std::min(D, cycle_depth(sims[i], hmin));
    }
    int left = n_steps;
    if (D && left >= D) {
        const HaloTables &T = cycle_halo(D);
        // The halo cycle of lb_run (full cycles + a lone first half) with the transport replaced: every member packs its edges on its
        // edge stream, the receivers unpack straight from the senders' buffers.
        for (int i = 0; i < count; ++i)
            if (!sims[i]->halo_buf) {
                HIP_TRY(hipMalloc(&sims[i]->halo_buf, sizeof(float) * 4 * HALO_SEGS_DEEP * sims[i]->p.nx));
                sims[i]->bytes += sizeof(float) * 4 * HALO_SEGS_DEEP * sims[i]->p.nx;
            }
        const size_t n = (size_t)T.n * sims[0]->p.nx;
        auto south_of = [&](int i) { return i > 0 ? i - 1 : (wrap ? count - 1 : -1); };
        auto north_of = [&](int i) { return i < count - 1 ? i + 1 : (wrap ? 0 : -1); };
        auto exchange_deep = [&]() -> int {
            for (int i = 0; i < count; ++i) {
                lb_sim *me = sims[i];
                // my send buffers are free again once both neighbours have unpacked the previous halo
                for (int nb : {south_of(i), north_of(i)})
                    if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->edge_stream, sims[nb]->ev_halo, 0));
                if ((rc = halo_pack(me, me->cur, me->edge_stream, T, north_of(i) >= 0, south_of(i) >= 0))) return rc;
                HIP_TRY(hipEventRecord(me->ev_packed, me->edge_stream));
            }
            for (int i = 0; i < count; ++i) {
                lb_sim *me = sims[i];
                const int so = south_of(i), no = north_of(i);
                for (int nb : {so, no})
                    if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->edge_stream, sims[nb]->ev_packed, 0));
                // my south ghost rows <- what the southern neighbour sent north, and vice versa
                if ((rc = halo_unpack(me, me->cur, me->edge_stream, T, so >= 0 ? sims[so]->halo_buf : nullptr,
                                      no >= 0 ? sims[no]->halo_buf + n : nullptr)))
                    return rc;
                HIP_TRY(hipEventRecord(me->ev_halo, me->edge_stream));
            }
            return LB_OK;
        };
        if ((rc = exchange_deep())) return rc;
        DBG_SYNC(2);
        for (; left >= 2 * D; left -= 2 * D) {
            for (int i = 0; i < count; ++i) {
                if ((rc = slab_cycle_first(sims[i], D))) return rc;
                sims[i]->cur ^= 1;
            }
            DBG_SYNC(1);
            for (int i = 0; i < count; ++i) {
                if ((rc = slab_cycle_second(sims[i], left == 2 * D, D))) return rc;
                sims[i]->cur ^= 1;
            }
            DBG_SYNC(1);
            if ((rc = exchange_deep())) return rc;
            DBG_SYNC(2);
            for (int i = 0; i < count; ++i) HIP_TRY(hipStreamWaitEvent(sims[i]->stream, sims[i]->ev_boundary, 0));
        }
        int depth_after = 2 * D;
        if (left >= D) {                            // the lone first half (see lb_run)
            const bool last = (left == D);
            for (int i = 0; i < count; ++i) {
                if ((rc = slab_cycle_first(sims[i], D, last))) return rc;
                sims[i]->cur ^= 1;
            }
            left -= D;
            depth_after = last ? 0 : D;
        }
        // (verification path: a plain join before whatever follows)
        for (int i = 0; i < count; ++i) {
            HIP_TRY(hipStreamSynchronize(sims[i]->edge_stream));
            HIP_TRY(hipStreamSynchronize(sims[i]->stream));
            sims[i]->ghost_depth = depth_after;
            sims[i]->feq_valid = false;
            sims[i]->macro_valid = !lazy_macro(sims[i]);
        }
        if (left == 0) return LB_OK;
        for (int i = 0; i < count; ++i) {
            HIP_TRY(hipEventRecord(sims[i]->ev_interior, sims[i]->stream));
            HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[i]->ev_interior, 0));
        }
    }
    if ((rc = exchange(0, false))) return rc;
    DBG_SYNC(2);
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipStreamWaitEvent(sims[i]->stream, sims[i]->ev_halo, 0));
        HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[i]->ev_halo, 0));
    }
    while (left > 0) {
        const int adv = next_advance(sims[0], depth_mask(two, three), left);
        for (int i = 0; i < count; ++i)
            if ((rc = slab_step_launch(sims[i], adv, left == adv))) return rc;
        DBG_SYNC(1);
        if ((rc = exchange(1, true))) return rc;
        DBG_SYNC(2);
        for (int i = 0; i < count; ++i) {
            if ((rc = slab_step_join(sims[i]))) return rc;
            // a neighbour's next launch overwrites the lattice my comm stream may still be reading
            // from (its old lattice): make every member wait for every halo copy that reads it
            const int south = i > 0 ? i - 1 : (wrap ? count - 1 : -1);
            const int north = i < count - 1 ? i + 1 : (wrap ? 0 : -1);
            for (int nb : {south, north}) {
                if (nb < 0) continue;
                HIP_TRY(hipStreamWaitEvent(sims[i]->stream, sims[nb]->ev_halo, 0));
                HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[nb]->ev_halo, 0));
            }
        }
        for (int i = 0; i < count; ++i) sims[i]->cur ^= 1;
        left -= adv;
        DBG_SYNC(4);
    }
    for (int i = 0; i < count; ++i) {
        sims[i]->ghost_depth = 3;
        sims[i]->feq_valid = false;
        sims[i]->macro_valid = !lazy_macro(sims[i]);
    }
    DBG_SYNC(8);
    return LB_OK;
}

// Population sets: `count` periodic whole-grid lattices of one geometry (one per population of a multi-population
// model, each with its own omega / mask content) advanced in lock step, ONE launch per time step for all of them.
int lb_run_batch(lb_sim **sims, int count, int n_steps)
{
    for (int i = 0; sims && i < count; ++i) CPU_UNSUPPORTED(sims[i], "lb_run_batch");
    if (!sims || count < 1 || count > BATCH_MAX || n_steps < 0)
        return fail(LB_ERR_ARG, "lb_run_batch takes 1..%d handles and a non-negative step count", BATCH_MAX);
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
    DeviceGuard guard(s0->p.device);
    // everything is enqueued on the first member's stream, behind whatever the others still have in flight
    for (int i = 1; i < count; ++i) {
        HIP_TRY(hipEventRecord(sims[i]->ev_interior, sims[i]->stream));
        HIP_TRY(hipStreamWaitEvent(s0->stream, sims[i]->ev_interior, 0));
    }
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
    // the other members' streams see the result
    HIP_TRY(hipEventRecord(s0->ev_interior, s0->stream));
    for (int i = 0; i < count; ++i) {
        if (i) HIP_TRY(hipStreamWaitEvent(sims[i]->stream, s0->ev_interior, 0));
        sims[i]->feq_valid = false;
        sims[i]->macro_valid = !lazy;
    }
    return LB_OK;
}

// ---- RCCL --------------------------------------------------------------------------------
int lb_comm_available(void) { return rccl_load(); }

int lb_comm_unique_id(void *unique_id_128)
{
    if (!unique_id_128) return fail(LB_ERR_ARG, "null argument");
    int rc = rccl_load();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(unique_id_128, &id, sizeof(id));
    return LB_OK;
}

int lb_comm_init(lb_sim *s, const void *unique_id_128, int rank, int nranks)
{
    CPU_UNSUPPORTED(s, "lb_comm_init");
    if (!s || !unique_id_128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(LB_ERR_ARG, "bad argument");
    int rc = rccl_load();
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    ncclUniqueId id;
    memcpy(&id, unique_id_128, sizeof(id));
    if (!s->halo_buf) {
        HIP_TRY(hipMalloc(&s->halo_buf, sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx));
        s->bytes += sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx;
    }
    // (RCCL's channel count.  Left alone, RCCL spreads the two sends and receives of an exchange -- 14 rows x 3 populations per direction,
    //  ~1.4 MB at 8192 columns -- over 59 workgroups of 256 threads with 20-37 KB of LDS each; k_deep's workgroups hold a CU's whole LDS
    //  in pairs, so those 59 trickle in as slots come free, sit on the SIMDs of an issue-bound kernel for most of a launch and take slots
    //  from the band launch behind them: one slab of four of an 8192^2 lattice 381 k MLUPS, with NCCL_MAX_NCHANNELS=2..16 438-450 k
    //  (profiles/r06c_slab_proxy_channels.txt, timeline profiles/r06c_slab_timeline_rccl_4.txt).  The per-communicator form of that cap,
    //  ncclConfig_t::maxCTAs through ncclCommInitRankConfig, is accepted and IGNORED by RCCL 2.26 / 2.27 (59 workgroups still:
    //  profiles/r06c_slab_timeline_rccl_4_cap8.txt), and the environment variable is read once per process at the first communicator's
    //  creation -- usually the caller's.  So the cap is the caller's to set before anything touches RCCL; neither this library nor
    //  bench.py sets it, and INTEGRATION.md explains why RCCL's default is left alone.)
    NCCL_TRY(g_rccl.CommInitRank(&s->comm, nranks, id, rank));
    s->rank = rank;
    s->nranks = nranks;
    // Which fused kernels a slab can run depends on its height; neighbours must exchange in the same
    // rhythm, so the ranks agree on the smallest height once, here.
    {
        int *d = reinterpret_cast<int *>(s->halo_buf);
        HIP_TRY(hipMemcpyAsync(d, &s->H, sizeof(int), hipMemcpyHostToDevice, s->edge_stream));
        NCCL_TRY(g_rccl.AllReduce(d, d + 1, 1, ncclInt32, ncclMin, s->comm, s->edge_stream));
        HIP_TRY(hipMemcpyAsync(&s->min_h, d + 1, sizeof(int), hipMemcpyDeviceToHost, s->edge_stream));
        HIP_TRY(hipStreamSynchronize(s->edge_stream));
    }
    s->ghost_depth = 0;
    return LB_OK;
}

// ---- peer transport ----------------------------------------------------------------------
namespace {
struct PeerDesc {                      // what lb_peer_export hands out (<= LB_PEER_HANDLE_BYTES)
    uint32_t magic, version;
    int32_t pid, device;
    int32_t nx, ny, h, planar;
    int64_t pitch, rowp, plane, lat_floats;
    uint64_t self_lat[2], self_flags;  // the exporter's own pointers: meaningful inside the exporting process only
    hipIpcMemHandle_t lat[2], flags;
};
static_assert(sizeof(PeerDesc) <= LB_PEER_HANDLE_BYTES, "LB_PEER_HANDLE_BYTES too small");
constexpr uint32_t PEER_MAGIC = 0x4c425052u;    // "LBPR"
}  // namespace

int lb_peer_export(lb_sim *s, void *handle_out)
{
    CPU_UNSUPPORTED(s, "lb_peer_export");
    if (!s || !handle_out) return fail(LB_ERR_ARG, "null argument");
    if (!s->multi_slab()) return fail(LB_ERR_STATE, "lb_peer_export needs a slab handle (LB_FLAG_HALO)");
    DeviceGuard guard(s->p.device);
    if (!s->peer_flags) {
        // fine-grained device memory: the neighbours' system-scope stores must become visible to a kernel that is already
        // running here (the bulk rows, ordinary coarse-grained memory, only have to be visible at kernel boundaries)
        void *f = nullptr;
        const size_t bytes = sizeof(unsigned long long) * PEER_FLAG_WORDS;
        if (hipExtMallocWithFlags(&f, bytes, hipDeviceMallocFinegrained) == hipSuccess) s->peer_flags_fine = true;
        else {
            (void)hipGetLastError();
            HIP_TRY(hipMalloc(&f, bytes));
        }
        s->peer_flags = static_cast<unsigned long long *>(f);
        HIP_TRY(hipMemset(s->peer_flags, 0, bytes));
    }
    PeerDesc d;
    memset(&d, 0, sizeof(d));
    d.magic = PEER_MAGIC; d.version = LB_ABI_VERSION;
    d.pid = (int32_t)getpid(); d.device = s->p.device;
    d.nx = s->p.nx; d.ny = s->p.ny; d.h = s->H; d.planar = (s->p.flags & LB_FLAG_PLANAR) ? 1 : 0;
    d.pitch = s->pitch; d.rowp = s->rowp; d.plane = s->plane; d.lat_floats = s->lat_floats;
    d.self_lat[0] = (uint64_t)(uintptr_t)s->lat[0]; d.self_lat[1] = (uint64_t)(uintptr_t)s->lat[1];
    d.self_flags = (uint64_t)(uintptr_t)s->peer_flags;
    HIP_TRY(hipIpcGetMemHandle(&d.lat[0], s->lat[0]));
    HIP_TRY(hipIpcGetMemHandle(&d.lat[1], s->lat[1]));
    if (hipIpcGetMemHandle(&d.flags, s->peer_flags) != hipSuccess && s->peer_flags_fine) {
        // (a runtime that cannot export fine-grained memory: fall back to an ordinary allocation -- enough between processes
        //  that share one GPU, where the flags meet in that GPU's own memory)
        (void)hipGetLastError();
        (void)hipFree(s->peer_flags);
        s->peer_flags = nullptr;
        s->peer_flags_fine = false;
        void *f = nullptr;
        HIP_TRY(hipMalloc(&f, sizeof(unsigned long long) * PEER_FLAG_WORDS));
        s->peer_flags = static_cast<unsigned long long *>(f);
        HIP_TRY(hipMemset(s->peer_flags, 0, sizeof(unsigned long long) * PEER_FLAG_WORDS));
        d.self_flags = (uint64_t)(uintptr_t)s->peer_flags;
        HIP_TRY(hipIpcGetMemHandle(&d.flags, s->peer_flags));
    }
    memset(handle_out, 0, LB_PEER_HANDLE_BYTES);
    memcpy(handle_out, &d, sizeof(d));
    return LB_OK;
}

int lb_peer_connect(lb_sim *s, int rank, int nranks, const void *south_handle, const void *north_handle, int min_h)
{
    CPU_UNSUPPORTED(s, "lb_peer_connect");
    if (!s || nranks < 1 || rank < 0 || rank >= nranks || min_h < 1) return fail(LB_ERR_ARG, "bad argument");
    if (!s->peer_flags) return fail(LB_ERR_STATE, "lb_peer_connect before lb_peer_export");
    if (s->peer_connected || s->comm) return fail(LB_ERR_STATE, "this handle already has a halo transport");
    DeviceGuard guard(s->p.device);
    const void *handles[2] = {south_handle, north_handle};
    PeerDesc d[2];
    for (int side = 0; side < 2; ++side) {
        if (!handles[side]) continue;
        memcpy(&d[side], handles[side], sizeof(PeerDesc));
        const PeerDesc &e = d[side];
        if (e.magic != PEER_MAGIC || e.version != LB_ABI_VERSION)
            return fail(LB_ERR_ARG, "not a peer descriptor of this library version");
        if (e.nx != s->p.nx || e.ny != s->p.ny || e.pitch != s->pitch || e.planar != ((s->p.flags & LB_FLAG_PLANAR) ? 1 : 0))
            return fail(LB_ERR_ARG, "the %s neighbour's lattice has another geometry or layout", side ? "north" : "south");
    }
    for (int side = 0; side < 2; ++side) {
        lb_sim::PeerNb &nb = s->peer_nb[side];
        if (!handles[side]) continue;
        const PeerDesc &e = d[side];
        nb.plane = e.plane; nb.rowp = e.rowp; nb.h = e.h;
        if (e.pid == (int32_t)getpid()) {              // exported by this process (a ring that closes on itself): use it in place
            nb.flags = reinterpret_cast<unsigned long long *>((uintptr_t)e.self_flags);
            nb.lat_raw[0] = reinterpret_cast<float *>((uintptr_t)e.self_lat[0]);
            nb.lat_raw[1] = reinterpret_cast<float *>((uintptr_t)e.self_lat[1]);
            continue;
        }
        if (side == 1 && handles[0] && d[0].pid == e.pid && d[0].self_flags == e.self_flags) {
            // two ranks in a periodic box: both neighbours are the same peer; one mapping serves both sides
            nb.flags = s->peer_nb[0].flags; nb.lat_raw[0] = s->peer_nb[0].lat_raw[0]; nb.lat_raw[1] = s->peer_nb[0].lat_raw[1];
            continue;
        }
        void *m = nullptr;
        HIP_TRY(hipIpcOpenMemHandle(&m, e.flags, hipIpcMemLazyEnablePeerAccess));
        nb.flags = static_cast<unsigned long long *>(m);
        nb.mapped = true;
        for (int w = 0; w < 2; ++w) {
            HIP_TRY(hipIpcOpenMemHandle(&m, e.lat[w], hipIpcMemLazyEnablePeerAccess));
            nb.lat_raw[w] = static_cast<float *>(m);
        }
    }
    if (!s->halo_buf) {       // (lb_check's scratch and the launch-by-launch fallback share it with the RCCL path)
        HIP_TRY(hipMalloc(&s->halo_buf, sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx));
        s->bytes += sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx;
    }
    double timeout_s = 20.0;
    if (const char *t = getenv("LB_PEER_TIMEOUT_S")) timeout_s = atof(t) > 0 ? atof(t) : timeout_s;
    s->peer_timeout_ticks = (unsigned long long)(timeout_s * 1e8);         // s_memrealtime: 100 MHz
    s->rank = rank;
    s->nranks = nranks;
    s->min_h = min_h;
    s->ghost_depth = 0;
    s->peer_connected = true;
    return LB_OK;
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
            if (fabsf(r) <= 3.0e38f && fabsf(usq) <= 3.0e38f) { sum += (double)r; mx = fmaxf(mx, usq); }
            else ++bad;
        }
        if (n_nonfinite) *n_nonfinite = bad;
        if (max_mach) *max_mach = sqrtf(3.f * mx);
        if (sum_rho) *sum_rho = sum;
        return LB_OK;
    }
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_check inside a split step");
    if (across_ranks && !s->comm) return fail(LB_ERR_STATE, "lb_check across ranks needs lb_comm_init");
    DeviceGuard guard(s->p.device);
    // the pass that rebuilds rho, u, v reduces the same three numbers: one pass serves both when the fields are due
    int rc = macro_check_pass(s, !s->macro_valid && lazy_macro(s));
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

// ---- measurement -------------------------------------------------------------------------
int lb_plan_launches(lb_sim *s, int n_steps, int *depths, int max_launches)
{
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (n_steps < 0) return fail(LB_ERR_ARG, "negative step count");
    if (s->cpu || s->p.semantics == LB_SEM_CYTHON || s->multi_slab()) return LB_ERR_STATE;     // (whole-grid OpenCL-path GPU handles)
    const int allowed = whole_grid_depths(s);
    int n = 0;
    for (int left = n_steps; left > 0; ++n) {
        const int adv = next_advance(s, allowed, left);
        if (depths && n < max_launches) depths[n] = adv;
        left -= adv;
    }
    return n;
}

int lb_steps_per_launch(lb_sim *s)
{
    if (s && s->cpu) return 1;
    if (!s) return fail(LB_ERR_ARG, "null handle");
    int n = 1;
    if (s->p.semantics == LB_SEM_CYTHON) return cython_tiles(s) ? TILE_T : 1;
    if (!s->multi_slab()) {
        const int depths = whole_grid_depths(s);
        for (int d = 2; d <= MAX_DEPTH; ++d)
            if (depths & (1 << d)) n = d;
    } else {
        const int v = effective_variant(s);
        const int h = s->min_h > 0 ? s->min_h : s->H;
        if (cycle_depth(s, h)) n = cycle_depth(s, h);
        else if ((v & VAR_STEP3) && step3_applicable(s, h)) n = 3;
        else if ((v & VAR_STEP2) && step2_applicable(s, h)) n = 2;
    }
    return n;
}

int lb_autotune(lb_sim *s)
{
    if (s && s->cpu) return 0;                     // (one code path on the host: nothing to choose between)
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_autotune inside a split step");
    if (!autotune_applies(s)) return 0;                // nothing to choose between
    // (a forced variant fixes the kernels: every candidate would be timed as those, and the launch plan made from such costs is
    //  nonsense -- bench.py --variant 119137 planned twenty steps as 1 + 1 + 4 + 7 + 7)
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
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (s->stepping) return fail(LB_ERR_STATE, "lb_autotune_quick inside a split step");
    if (!s->tune_cache_checked && tune_cache_apply(s)) return 0;       // (LB_TUNE_CACHE: an earlier handle of this shape was tuned)
    if (!autotune_applies(s) || s->variant >= 0 || s->tuned_steps || max_steps < autotune_quick_cost(s)) return 0;
    DeviceGuard guard(s->p.device);
    return autotune_whole_grid(s, 1, max_steps);
}

int lb_hot_kernel(lb_sim *s, char *buf, int buflen)
{
    if (s && s->cpu) {
        if (!buf || buflen < 1) return fail(LB_ERR_ARG, "bad argument");
        snprintf(buf, (size_t)buflen, "cpu backend (cython_dim.pyx Pipe_Flow.run restated for the host, 1 thread)");
        return LB_OK;
    }
    if (!s || !buf || buflen < 1) return fail(LB_ERR_ARG, "bad argument");
    static const char *const bc_names[] = {"PIPE", "PERIODIC", "CAVITY", "VELOCITY_INLET", "PIPE, D2Q9i"};
    const char *kernel = "k_step";
    if (s->p.semantics == LB_SEM_CYTHON)
        kernel = cython_tiles(s) ? "k1_tile4 (Cython path, LDS tiles)" : "k1_fstep (Cython path)";
    else {
        const int spl = lb_steps_per_launch(s);
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
