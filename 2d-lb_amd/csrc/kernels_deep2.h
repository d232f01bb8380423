// kernels_deep2.h -- k_deep's march with TWO waves per strip and direction, so that two waves share every SIMD (round 6).
//
// Why.  k_deep runs one wave per SIMD -- 40 KB of LDS windows and ~280 registers per wave leave room for no second one -- and a lone
// wave issues one instruction per ~5 cycles whatever the instruction: the vector ALU is busy 65 % of the time, the launch is bound
// by instruction issue.  Round 5 priced a second wave per SIMD at "nothing" from two DIFFERENT kernels;
// round 6 ran the SAME kernel both ways (k_deep<4>, 213 registers, 16 KB: profiles/r06_occ2_probe.txt, 8192^2, arithmetic only, no
// global memory): four waves per CU 767 us per launch, eight waves per CU 415 us -- of which ~1.4 x is the second wave's doing (a
// quarter of the four-waves build's waves had doubled up on SIMDs and set its launch time: profiles/r06_occ2_placement.txt).  A SIMD fed
// by two waves issues their scalar, LDS and memory instructions beside the other's vector instructions and covers their stalls.
//
// How.  A wave's state must halve.  So the D stages of a strip's march are split between two waves that share the strip: the FRONT
// wave gathers the rows from memory (one row ahead, in a register window it waits for by hand: kernels_deep.h) and runs stages
// 1..F, the BACK wave runs stages F+1..D and stores.  Each is an ordinary k_deep march (kernels_deep.h: deep_iter with ROLE) of depth F
// / D - F + 1 -- the back wave's "step 1" being the row the front wave hands it through ONE 9.25 KB slot of LDS (nine links + the
// row's obstacle flags) --, with its own stage windows (registers + LDS) and its own partner of the other direction: a workgroup is
// four waves, front-down, front-up, back-down, back-up; the two front waves hand each other the links that cross the pair's middle
// line while their pipelines fill, and so do the two back waves, exactly as k_deep's two waves do.  The back waves run one trip
// behind the front waves.  Per trip, two workgroup barriers: (1) the back waves have taken the slot's row -- the front waves may
// overwrite it at the end of their iteration --, (2) the front waves' rows and everybody's published links are visible.
//
// Resources per wave at D = 7, F = 4: front 2 register windows + 1 LDS window (8 KB) + the slot its row gathered ahead is loaded
// into (10 KB: the row in flight is in NO register -- `buffer_load ... lds`, kernels_deep.h: deep_row_issue_lds); back 2 register windows
// + 1 LDS window (8 KB); the hand-over slot 10 KB per direction: 72 KB per workgroup, two workgroups = eight waves per CU; 256 vector
// registers per wave, no accumulation register.
//
// Roles.  Which of the four bodies a wave enters follows the SIMD it runs on, read at entry (deep2_take_role below, deep2_roles.h): every
// SIMD of a CU with two workgroups holds a front wave of one and a back wave of the other, 4 + 3 stage bodies per row.
//
// Issue priority.  Every front wave raises its priority once, at entry (deep2_set_prio below): without it the older of a CU's two
// workgroups is served first on every SIMD and the younger runs a quarter of the launch alone.
//
// Steady trips in pairs (deep2_pairs_front / deep2_pairs_back below).  Both roles keep two stage windows in registers, and in a loop
// whose body is one trip the values carried to the next trip sit in fixed registers: the row a stage has just produced is live beside
// the window the next stage still gathers from, so the compiler copies -- of the 121 register moves per row in the front loop and the 83 in the back loop
// 27 and 26 are of that kind and compute nothing.  With two trips per body the two names swap: a periodic box without a mask runs an unconditional paired loop
// while two more trips lie inside the wave's own positions (and inside `trips`), then the guarded single-trip loop for what is left --
// at most one more position of its own, then the other waves' trips.  Every trip, paired or not, executes the same two barriers, so
// the four waves of a workgroup stay matched whatever loop each is in (the halves of a pair differ by a row, the back waves run F
// trips behind).  Three things make the pair what it should be: deep2_settle (no scratch in the back wave), deep2_trip_fence (the
// back wave's work stays between its trip's barriers) and, in the front wave, deep_pair_typed (kernels_deep.h: stage 1's twenty scalar
// subtractions packed).  Per strip and row 1149 -> 1092.5 vector instructions (-4.9 %, profiles/deep2_pairs_isa.txt); on the device
// SQ_INSTS_VALU 3.236e8 -> 3.068e8 per 8192^2 launch (-5.2 %).  What that is worth in time, and which instantiations pair:
// deep2_pairs_front below, profiles/deep2_pairs_ab.txt.
//
// The launch moves the same 72 B per cell; same cell functions, same operations in the same order: bitwise equal to k_step.
#pragma once

#include "deep2_roles.h"

namespace {

// registers windows of the front / back wave, per depth and split (see the header)
constexpr int deep2_split(int D) { return D >= 8 ? 4 : (D + 1) / 2; }          // F: stages of the front wave (7 -> 4, 6 -> 3)
constexpr int deep2_rw_front(int D) { return deep2_split(D) - 2 >= 2 ? 2 : 1; }
constexpr int deep2_rw_back(int D) { return (D - deep2_split(D) + 1) - 2 >= 2 ? 2 : 1; }
constexpr int DEEP2_WAVES = 4;
// Which instantiations run their steady trips in pairs (see the header), per role.  Measured, 8192^2 periodic, 84 steps pinned to
// k_deep2<7>, five rounds alternated on one box, k MLUPS (profiles/deep2_pairs_ab.txt):
//     parent 510.7-511.9 | pair-typed stage 1 alone 511.9-512.5 | + front pairs 512.7-513.6 | + back pairs (this) 515.0-515.9
// every line of each step above every line of the step before; +0.8 % in all, for 5.2 % fewer vector instructions on the device: the
// launch does not follow its vector-instruction count the way its 82 % busy vector ALU suggested, what the waves wait for at the
// barriers grows by what they save (SQ_WAIT_ANY 1.82e8 -> 1.92e8 per launch, SQ_WAVE_CYCLES 8.15e8 -> 8.10e8).  The same pairs WITHOUT
// deep2_trip_fence: 456.8-459.6 against the parent's 505.0-505.4 on another box, -9.5 %.
// With walls or a mask neither role can be paired without scratch (both roles 80-224 B per lane, the front alone 80-192 B, where the
// parent has 0-64 B: profiles/deep2_pairs_isa.txt), so those instantiations stay as they were, instruction for instruction.
constexpr bool deep2_pairs_front(bool mask, int bc) { return !mask && bc == LB_BC_PERIODIC; }
constexpr bool deep2_pairs_back(bool mask, int bc) { return !mask && bc == LB_BC_PERIODIC; }

// The trip's two barriers (see the header).  NOT __syncthreads(): that is a fence as well -- `s_waitcnt vmcnt(0)` in front of the
// barrier --, and at every trip a back wave would wait out the nine stores it has just issued, a front wave the row it has just asked
// for: the whole workgroup stalls on memory latency twice per row (the first k_deep2, profiles/r06_deep2_first.txt: 0.92-0.95 ms per
// 8192^2 launch where k_deep<7> takes 0.89).  What the waves hand each other goes through LDS: an LDS instruction that has completed
// (lgkmcnt) is visible to the workgroup.
__device__ __forceinline__ void deep2_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// (a steady trip's: the diagnostic build can run the steady state without them -- timing only, races: wrong results)
__device__ __forceinline__ void deep2_steady_barrier(const StepArgs &a)
{
#ifdef LB_DIAG
    if (a.diag & (1 << 24)) return;
#endif
    deep2_barrier();
}

// Static issue priority by role.  The hardware gives a SIMD's vector issue to the higher priority, then to the OLDER wave: at equal
// priority the workgroup a CU was given first wins on all four SIMDs, runs as if alone and ends at three quarters of the launch, and
// the second runs the rest with one wave per SIMD.  One role raises its priority -- once, at entry, never inside the march.  With the
// roles taken by SIMD (deep2_take_role) every shared SIMD holds a front wave of one workgroup and a back wave of the other, so the
// raised role wins on every SIMD, each workgroup on two of the four, and with EITHER role raised a CU's two workgroups end within
// 0.1 % of the launch of each other (per-wave records, profiles/deep2_roles_ab.txt).  Which role is measured (8192^2 periodic, product
// builds alternated): with the FRONT waves raised the launch is 3-4 % shorter than with the back waves -- the front wave, four stages
// and the gather, sets its workgroup's pace at the barriers and is served first; the back wave, three stages, lives on what is left.
// (Under the static roles -- two front waves on one SIMD of four, where age decided -- it was the back waves:
// profiles/deep2_priority_ab.txt.)
// mode (StepArgs::deep2_prio): 0 none, 1 front waves, 2 back waves; the diagnostic build overrides it by LB_DIAG bits 25-26
// (0 = as launched, 1 / 2 / 3 = mode 0 / 1 / 2) so that one library runs the A/B.
__device__ __forceinline__ void deep2_set_prio(const StepArgs &a, const int role_mode)
{
    int mode = a.deep2_prio;
#ifdef LB_DIAG
    if ((a.diag >> 25) & 3) mode = ((a.diag >> 25) & 3) - 1;
#endif
    if (mode == role_mode) __builtin_amdgcn_s_setprio(1);
}

// ---- the front wave: stages 1..F of positions 0 .. len + D - 2, one per trip from trip 0 ---------------------------------------
template <int BC, bool MASK, int F, int RW, bool DOWN, int NST>
__device__ __forceinline__ void deep2_front_fill(const StepArgs &a, const DeepCtx &cx, DeepState<RW, F - 1 - RW> &st, Row1 &ra, Row1 &rb,
                                                 int &trip)
{
    if constexpr (NST < F) {
        deep2_barrier();
        if (trip < cx.n_iter) {
            if ((NST & 1) == 0) deep_iter<BC, MASK, false, F, RW, 1, DOWN, NST, -1, DEEP_FRONT>(a, cx, NST - 1, st, rb, ra);
            else deep_iter<BC, MASK, false, F, RW, 1, DOWN, NST, -1, DEEP_FRONT>(a, cx, NST - 1, st, ra, rb);
        }
        deep2_barrier();
        ++trip;
        deep2_front_fill<BC, MASK, F, RW, DOWN, NST + 1>(a, cx, st, ra, rb, trip);
    }
}

template <int BC, bool MASK, int D, int F, int RW, bool DOWN>
__device__ __forceinline__ void deep2_front(const StepArgs &a, const int x0, const int ym, const int len, const int trips, f4a (*mine)[64],
                                            f4a (*other)[64], f4a (*ho)[64], f4a (*dma)[64])
{
    deep2_set_prio(a, 1);
    DeepCtx cx;
    cx.lane = threadIdx.x;
    const int xr = x0 + cx.lane * 4;
    cx.x4 = skirt_column<BC>(a, xr, deep_skirt_lanes(D));
    cx.store_lane = false;                              // (a front wave stores nothing)
    cx.ym = ym; cx.n_iter = len + D - 1;                // every position the BACK wave's last stage needs
    cx.mine = mine; cx.other = other; cx.ho = ho; cx.dma = dma;
    // (a pointer into LDS as a 64-bit number: the aperture's base above, the byte offset inside the workgroup's LDS below)
    cx.dma_off = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<unsigned long long>(dma));
    DeepState<RW, F - 1 - RW> st = {};
    auto row_at = [&](int p) { return DOWN ? ym - 1 - p : ym + p; };
    Row1 ra, rb;
    deep_row_issue_lds<BC, MASK>(a, row_at(0), cx.x4, cx.dma_off, ra);
    int trip = 0;
    deep2_front_fill<BC, MASK, F, RW, DOWN, 1>(a, cx, st, ra, rb, trip);
    if constexpr (!deep2_pairs_front(MASK, BC)) {
        if ((F - 1) & 1) ra = rb;                       // (position F - 1 is in ra or rb by its parity)
        for (; trip < trips; ++trip) {
            deep2_steady_barrier(a);
            if (trip < cx.n_iter) {
                deep_iter<BC, MASK, false, F, RW, 1, DOWN, F, -1, DEEP_FRONT>(a, cx, trip, st, ra, rb);
                ra = rb;
            }
            deep2_steady_barrier(a);
        }
    } else {
        // position i is in ra for even i, in rb for odd i: the two buffers swap roles by argument order, the parity is a constant
        constexpr int P0 = (F - 1) & 1;
        Row1 &r0 = P0 ? rb : ra, &r1 = P0 ? ra : rb;
        const int paired = min(cx.n_iter, trips);
        for (; trip + 1 < paired; trip += 2) {
            deep2_steady_barrier(a);
            deep_iter<BC, MASK, false, F, RW, 1, DOWN, F, P0, DEEP_FRONT>(a, cx, trip, st, r0, r1);
            deep2_steady_barrier(a);
            deep2_steady_barrier(a);
            deep_iter<BC, MASK, false, F, RW, 1, DOWN, F, 1 - P0, DEEP_FRONT>(a, cx, trip + 1, st, r1, r0);
            deep2_steady_barrier(a);
        }
        // the rest: at most one more position of mine (trip + 1 >= n_iter: the parity is still P0), then the other waves' trips
        for (; trip < trips; ++trip) {
            deep2_steady_barrier(a);
            if (trip < cx.n_iter) deep_iter<BC, MASK, false, F, RW, 1, DOWN, F, P0, DEEP_FRONT>(a, cx, trip, st, r0, r1);
            deep2_steady_barrier(a);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the row gathered behind the last position)
}

// ---- the back wave: stages F+1..D, one trip behind: its iteration j (position j enters) runs in trip j + F ------------------------
template <bool MASK>
__device__ __forceinline__ void deep2_take(const DeepCtx &cx, Row1 &cur)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) cur.q[k] = cx.ho[k][cx.lane];
    cur.mk = uc4{0, 0, 0, 0};
    if (MASK) cur.mk = __builtin_bit_cast(uc4, reinterpret_cast<const unsigned *>(cx.ho[9])[cx.lane]);
    cur.have = true;
}

// Between the two trips of a pair (deep2_back below).  A stage's row enters the next register window for the trips to come; nothing in
// its own trip reads more of it than the three links pulled from ahead.  In a rolled loop the row is in the window's registers at the
// back edge.  With two trips in one body the compiler sinks the row's last nine fma below the trip's stores, into the next trip, and
// keeps their operands -- the row before relaxation and its equilibria, twice the registers -- live across the barrier and the take:
// 152 B of scratch per lane, 17 scratch instructions per pair.  An empty asm on the windows' d and e rows ends the trip for them: no
// scratch, 250 registers as before.  (Window 1 takes the row handed over, a load: nothing to sink; of an LDS window's row only link 0
// stays in registers.)
template <int RW, int NL>
__device__ __forceinline__ void deep2_settle(DeepState<RW, NL> &st)
{
#pragma unroll
    for (int k = 1; k < RW; ++k) {
        Window &w = st.w[k];
        asm volatile("" : "+v"(w.d0), "+v"(w.d1), "+v"(w.d3), "+v"(w.e2), "+v"(w.e5), "+v"(w.e6));
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) asm volatile("" : "+v"(st.d0[k]));
}

// Around a paired trip's work (deep2_back below).  The barriers are asm statements: vector instructions move across them freely.  In
// the rolled loop the back edge keeps a trip's work between its two barriers and leaves the take alone between the second and the
// next first (30 instructions).  In a two-trip body the scheduler sinks the tail of one trip and hoists the head of the next into
// that gap, 163 and 79 instructions -- which the front waves, who have nothing to do there, spend waiting at the first barrier:
// SQ_WAIT_ANY 1.83e8 -> 4.23e8 per 8192^2 launch, the launch 9.5 % LONGER with 5.2 % fewer vector instructions
// (profiles/deep2_pairs_ab.txt section 1).  A scheduling fence behind the first barrier and in front of the second: 11 and 16.
__device__ __forceinline__ void deep2_trip_fence() { __builtin_amdgcn_sched_barrier(0); }

template <int BC, bool MASK, bool MACRO, int DB, int RW, bool DOWN, int NST>
__device__ __forceinline__ void deep2_back_fill(const StepArgs &a, const DeepCtx &cx, DeepState<RW, DB - 1 - RW> &st, Row1 &cur, int &j)
{
    if constexpr (NST < DB) {
        if (j < cx.n_iter) deep2_take<MASK>(cx, cur);
        deep2_barrier();
        if (j < cx.n_iter) deep_iter<BC, MASK, MACRO, DB, RW, 0, DOWN, NST, -1, DEEP_BACK>(a, cx, NST - 1, st, cur, cur);
        deep2_barrier();
        ++j;
        deep2_back_fill<BC, MASK, MACRO, DB, RW, DOWN, NST + 1>(a, cx, st, cur, j);
    }
}

template <int BC, bool MASK, bool MACRO, int D, int F, int RW, bool DOWN>
__device__ __forceinline__ void deep2_back(const StepArgs &a, const int x0, const int ym, const int len, const int trips, f4a (*mine)[64],
                                           f4a (*other)[64], f4a (*ho)[64])
{
    constexpr int DB = D - F + 1;                       // the back wave's own depth: "step 1" = the row handed over
    deep2_set_prio(a, 2);
    DeepCtx cx;
    cx.lane = threadIdx.x;
    const int xr = x0 + cx.lane * 4;
    cx.x4 = skirt_column<BC>(a, xr, deep_skirt_lanes(D));
    cx.store_lane = skirt_store_lane(a, cx.lane, xr, deep_skirt_lanes(D));
    cx.ym = ym; cx.n_iter = len + DB - 1;
    cx.mine = mine; cx.other = other; cx.ho = ho;
    DeepState<RW, DB - 1 - RW> st = {};
    Row1 cur;
    cur.wp = WrapPatch{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    cur.hsolid = false; cur.hxc = -1; cur.rr = 0;
    // trips 0 .. F - 1: the front wave's pipeline fills, nothing has been handed over yet
    for (int t = 0; t < F; ++t) {
        deep2_barrier();
        deep2_barrier();
    }
    int j = 0;
    deep2_back_fill<BC, MASK, MACRO, DB, RW, DOWN, 1>(a, cx, st, cur, j);
    if constexpr (deep2_pairs_back(MASK, BC)) {
        constexpr int P0 = (DB - 1) & 1;
        const int paired = min(cx.n_iter, trips - F);
        for (; j + 1 < paired; j += 2) {
            deep2_take<MASK>(cx, cur);
            deep2_steady_barrier(a);
            deep2_trip_fence();
            deep_iter<BC, MASK, MACRO, DB, RW, 0, DOWN, DB, P0, DEEP_BACK>(a, cx, j, st, cur, cur);
            deep2_settle(st);
            deep2_trip_fence();
            deep2_steady_barrier(a);
            deep2_take<MASK>(cx, cur);
            deep2_steady_barrier(a);
            deep2_trip_fence();
            deep_iter<BC, MASK, MACRO, DB, RW, 0, DOWN, DB, 1 - P0, DEEP_BACK>(a, cx, j + 1, st, cur, cur);
            deep2_trip_fence();
            deep2_steady_barrier(a);
        }
    }
    // (behind a paired loop: at most one more position of mine, then the other waves' trips)
    for (; j + F < trips; ++j) {
        if (j < cx.n_iter) deep2_take<MASK>(cx, cur);
        deep2_steady_barrier(a);
        if (j < cx.n_iter) deep_iter<BC, MASK, MACRO, DB, RW, 0, DOWN, DB, -1, DEEP_BACK>(a, cx, j, st, cur, cur);
        deep2_steady_barrier(a);
    }
}

// ---- which of the four bodies a wave enters: 0 front-down, 1 front-up, 2 back-down, 3 back-up ------------------------------------
// A front wave issues four stage bodies and the gather per row, a back wave three and the stores; a CU holds two workgroups, every
// SIMD two waves, and both workgroups advance at the pace of their slowest wave (two barriers per row).  Each SIMD should therefore
// hold a front wave of one workgroup and a back wave of the other: 4 + 3 stage bodies per row on every SIMD.
//
// The static rule (deep2_static_role: the wave's number, two on for every other 256 workgroups) assumes that wave w of every
// workgroup lands on SIMD w.  It does not: the per-wave records (tools/wave_timeline.py, profiles/deep2_priority_ab.txt section 1) have a
// front and a back wave on two SIMDs of a CU, two front waves on one -- 8 stage bodies and two gathers per row, and BOTH workgroups
// have a wave there -- and two back waves on one.
//
// By SIMD: every wave reads the SIMD it runs on (HW_REG_HW_ID, bits 5:4), lane 0 publishes it in one LDS word per wave, and behind one
// barrier every wave works out all four roles from the same four words (deep2_roles.h: deep2_assign_roles -- a permutation of 0..3
// whatever the words hold) and takes its own.  `flip` tells the two workgroups of a CU apart: the launch-order bit
// (blockIdx.x >> 8) & 1 -- they are 256 apart in launch order.  Measured (profiles/deep2_roles_ab.txt): opposite on every CU of the 8192^2
// periodic launch, of a walled one with edge items and of a 512-workgroup one, a front and a back wave on every shared SIMD.  Where it
// failed to, that CU would hold two fronts on two SIMDs and two backs on two: slower, never wrong.
//
// The diagnostic build runs the A/B from one library: LB_DIAG bit 27 = the static rule, exactly the code it was; bits 28-29 = 2 / 3:
// another flip signal, taken from wave 0's hardware state and published in bit 2 of its word -- 2 = its wave-slot parity (HW_ID bit
// 0, the bit k_step5 reads), 3 = the workgroup's LDS does not start at the CU's (HW_REG_LDS_ALLOC: its base).  Both measured as good as
// the launch-order bit, neither better.
__device__ __forceinline__ int deep2_take_role(const StepArgs &a, unsigned *lds_role, unsigned &note)
{
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int launch_flip = (blockIdx.x >> 8) & 1;
    int sig = 1;
#ifdef LB_DIAG
    if (a.diag & (1 << 27)) {
        note = (unsigned)launch_flip << 30;
        return deep2_static_role(w, launch_flip);
    }
    if ((a.diag >> 28) & 3) sig = (a.diag >> 28) & 3;
#endif
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID: wave_id[3:0] simd_id[5:4]
    unsigned word = (hw >> 4) & 3u;
    if (sig == 2) word |= (hw & 1u) << 2;
    if (sig == 3) word |= (__builtin_amdgcn_s_getreg((31 << 11) | 6) & 0xfffu) ? 4u : 0u;      // HW_REG_LDS_ALLOC: lds_base in the low bits
    if (threadIdx.x == 0) lds_role[w] = word;
    deep2_barrier();
    int simd[DEEP2_WAVES], role[DEEP2_WAVES];
    unsigned word0 = 0;
#pragma unroll
    for (int k = 0; k < DEEP2_WAVES; ++k) {
        const unsigned v = __builtin_amdgcn_readfirstlane(lds_role[k]);
        simd[k] = (int)(v & 3u);
        if (k == 0) word0 = v;
    }
    const int flip = sig == 1 ? launch_flip : (int)((word0 >> 2) & 1u);
    deep2_assign_roles(simd, flip, role);
    note = ((unsigned)flip << 30) | (1u << 29);
    return w == 0 ? role[0] : (w == 1 ? role[1] : (w == 2 ? role[2] : role[3]));     // (no indexed register array: no scratch)
}

// Launch geometry as k_deep: one workgroup = one segment pair of one strip, now four waves; XCD-transposed order, shorter segments for
// the two wall-column strips.  LDS: front 2 x (F - 1 - RWF) windows, back 2 x (D - F - RWB) windows, 2 slots.
template <int BC, bool MASK, bool MACRO, int D>
__global__ __launch_bounds__(64 * DEEP2_WAVES, 2) void k_deep2(const StepArgs a, int strips, int seg_rows, int nsegs, int row_end)
{
    constexpr int F = deep2_split(D), RWF = deep2_rw_front(D), RWB = deep2_rw_back(D);
    constexpr int LF = (F - 1 - RWF) * DEEP_WSLOTS, LBK = (D - F - RWB) * DEEP_WSLOTS;
    static_assert(2 * (LF + LBK + 2 * DEEP_HO_SLOTS) <= 80, "two workgroups per CU: 80 KB each");
    __shared__ f4a lds_dma[2][DEEP_HO_SLOTS][64];
    __shared__ f4a lds_front[2][LF][64];
    __shared__ f4a lds_back[2][LBK][64];
    __shared__ f4a lds_ho[2][DEEP_HO_SLOTS][64];
    __shared__ unsigned lds_role[DEEP2_WAVES];          // what each wave reports of where it runs (deep2_take_role)
    const int item = xcd_item(blockIdx.x, gridDim.x);
#ifdef LB_DIAG
    const unsigned long long diag_t0 = __builtin_amdgcn_s_memrealtime();     // 100 MHz
#endif
    int sx, sy;
    if (item < strips * nsegs) {
        sx = item % strips;
        sy = item / strips;
    } else {
        if (!a.edge_seg_rows) return;
        const int j = item - strips * nsegs;
        sx = (j & 1) ? strips - 1 : 0;
        sy = nsegs + (j >> 1);
    }
    int stride = a.seg_stride;
    if (a.edge_seg_rows && (sx == 0 || sx == strips - 1)) stride = seg_rows = a.edge_seg_rows;
    const int ya = a.row_begin + sy * stride;
    if (ya >= row_end) return;                          // (all four waves of the workgroup: the barriers stay matched)
    const int yb = min(ya + seg_rows, row_end);
    const int ym = ya + (yb - ya) / 2;                  // the pair's middle line: the down waves march down from it, the up waves up
    const int x0 = sx * deep_valid(D) - 4 * deep_skirt_lanes(D);
    const int trips = max(ym - ya, yb - ym) + D;        // front: len + D - 1 iterations from trip 0; back: len + D - F from trip F
    unsigned role_note = 0;
    const int wy = deep2_take_role(a, lds_role, role_note);       // (behind the two returns above: its barrier is the whole workgroup's)
    if (wy == 0) deep2_front<BC, MASK, D, F, RWF, true>(a, x0, ym, ym - ya, trips, lds_front[0], lds_front[1], lds_ho[0], lds_dma[0]);
    else if (wy == 1) deep2_front<BC, MASK, D, F, RWF, false>(a, x0, ym, yb - ym, trips, lds_front[1], lds_front[0], lds_ho[1], lds_dma[1]);
    else if (wy == 2) deep2_back<BC, MASK, MACRO, D, F, RWB, true>(a, x0, ym, ym - ya, trips, lds_back[0], lds_back[1], lds_ho[0]);
    else deep2_back<BC, MASK, MACRO, D, F, RWB, false>(a, x0, ym, yb - ym, trips, lds_back[1], lds_back[0], lds_ho[1]);
#ifdef LB_DIAG
    if ((a.diag & 4096) && threadIdx.x == 0) {
        // per-wave timeline as k_deep's (tools/wave_timeline.py, LB_TIMELINE_DEEP2=1): four records per item; [6] = item * 4 + role
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        unsigned *o = reinterpret_cast<unsigned *>(a.rho) + 8 * (item * DEEP2_WAVES + wy);
        o[0] = (unsigned)diag_t0; o[1] = (unsigned)(diag_t0 >> 32); o[2] = (unsigned)t1; o[3] = (unsigned)(t1 >> 32);
        o[4] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // HW_REG_XCC_ID
        o[5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_REG_HW_ID
        // [6]: the role TAKEN; [7]: the march's rows, bit 30 = the workgroup's flip, bit 29 = roles by SIMD (deep2_take_role)
        o[6] = (unsigned)(item * DEEP2_WAVES + wy); o[7] = (unsigned)((wy & 1) ? yb - ym : ym - ya) | role_note;
    }
#endif
}

}  // namespace
