// slab.cpp -- a row slab of a lattice that several handles share: the halo tables, pack / unpack, the exchange over RCCL and over the
// peer transport, the launch-by-launch schedule and the halo cycle of lb_run on a slab, lb_run_group (the same schedule on one device,
// for verification), lb_step_* and lb_halo_* (the caller drives the steps and moves the halo himself).
#include "host.h"
#include "kernels_halo.h"

const size_t peer_flag_bytes = sizeof(unsigned long long) * PEER_FLAG_WORDS;

namespace {

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
    const int rc = s->peer_connected() ? exchange_peer(s, which, q, T) : exchange_rccl(s, which, q, T);
    if (timed && !rc) {
        HIP_TRY(hipEventRecord(s->xt_ev[2 * s->xt_count + 1], q));
        ++s->xt_count;
    }
    return rc;
}

}  // namespace

// a wait of the peer transport gave up (the neighbour never arrived): reported once the device is idle
int peer_check_error(lb_sim *s)
{
    if (!s->peer_connected()) return LB_OK;
    unsigned long long err = 0;
    HIP_TRY(hipMemcpy(&err, s->peer_flags + PEER_ERR, sizeof(err), hipMemcpyDeviceToHost));
    if (err)
        return fail(LB_ERR_COMM, "peer transport: a neighbour did not arrive at halo exchange %llu within the timeout "
                                 "(LB_PEER_TIMEOUT_S); the state of this handle is not valid", err);
    return LB_OK;
}

int ensure_halo_buf(lb_sim *s)
{
    if (s->halo_buf) return LB_OK;
    HIP_TRY(hipMalloc(&s->halo_buf, sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx));
    s->bytes += sizeof(float) * 4 * HALO_SEGS_DEEP * s->p.nx;
    return LB_OK;
}

namespace {

// bands of output rows [lo_s, hi_s) and [lo_n, hi_n): one wave per strip and band
int launch_bands(lb_sim *s, hipStream_t st, int lo_s, int hi_s, int lo_n, int hi_n, bool macro, int depth)
{
    MarchRows r;
    r.stream = st; r.depth = depth; r.macro = macro;
    if (hi_s - lo_s == hi_n - lo_n) {               // one launch: two segments lo_n - lo_s apart
        r.row_begin = lo_s; r.row_end = hi_n;
        r.bands.count = 2; r.bands.rows = hi_s - lo_s; r.bands.stride = lo_n - lo_s;
        return launch_marching(s, r);
    }
    r.bands.count = 1;
    r.row_begin = lo_s; r.row_end = hi_s; r.bands.rows = hi_s - lo_s;
    int rc = launch_marching(s, r);
    r.row_begin = lo_n; r.row_end = hi_n; r.bands.rows = hi_n - lo_n;
    if (!rc) rc = launch_marching(s, r);
    return rc;
}

// the rows [lo, hi) between the bands, on the compute stream, in one balanced round of the wave slots the band launch beside it
// leaves: two bands x strips items, two waves each from k_step4 on
int launch_interior(lb_sim *s, int lo, int hi, bool macro, int depth)
{
    MarchRows r;
    r.stream = s->stream; r.row_begin = lo; r.row_end = hi; r.depth = depth; r.macro = macro;
    r.reserve = 2 * march_strips(s->p.nx, depth) * (depth >= 4 ? STEP4_WAVES : 1);
    return launch_marching(s, r);
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
        // edge bands: output rows [0,3) and [H-3,H), one wave per strip and band
        if ((rc = launch_bands(s, s->edge_stream, 0, 3, H - 3, H, macro, adv))) return rc;
        HIP_TRY(hipEventRecord(s->ev_boundary, s->edge_stream));
        if ((rc = launch_interior(s, 3, H - 3, macro, adv))) return rc;
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

const HaloTables &cycle_halo(int depth)
{
    return depth == 7 ? HALO14 : (depth == 6 ? HALO12 : (depth == 5 ? HALO10 : (depth == 4 ? HALO8 : HALO6)));
}

// E1 + C1 (the caller flips cur afterwards); D = depth of the fused kernel (3 or 4).  last = this launch ends the run:
// rho,u,v are stored and the ghost rows are not recomputed (nothing will consume them; the MACRO epilogue has no rows
// outside the slab to write to).  split: the bands in two launches, the outer one behind the exchange on the communication
// stream (ev_halo); else the caller has put the exchange on the edge stream itself.
int slab_cycle_first(lb_sim *s, int D, bool last = false, bool split = false)
{
    const int H = s->H;
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
    if ((rc = launch_interior(s, D + B, H - D - B, macro, D))) return rc;
    HIP_TRY(hipEventRecord(s->ev_interior, s->stream));
    return LB_OK;
}

// E2 + C2 (the caller flips cur afterwards); ev_edge = the 2D edge rows of the new lattice are complete (the exchange may start),
// ev_boundary = all of the bands' rows are (the next C1 may)
int slab_cycle_second(lb_sim *s, bool macro, int D, bool split = false)
{
    const int H = s->H;
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
    return launch_interior(s, 2 * D + B, H - 2 * D - B, macro, D);
}

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

// lb_run on a slab handle
int run_slab(lb_sim *s, int n_steps)
{
    int rc;
    if (!s->comm && !s->peer_connected())
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
    const int hmin = s->agreed_h();     // all ranks decide on the same height
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
    const int step_depths = slab_step_depths(s, hmin);
    const bool stepped = left > 0;
    while (left > 0) {
        const int adv = next_advance(s, step_depths, left);
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

extern "C" {

// ---- fused stepping ----------------------------------------------------------------------
int lb_step_boundary(lb_sim *s, int write_macro)
{
    CPU_UNSUPPORTED(s, "lb_step_boundary");
    SCALAR_UNSUPPORTED(s, "lb_step_boundary");
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
    SCALAR_UNSUPPORTED(s, "lb_step_interior");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    if (!s->stepping) return fail(LB_ERR_STATE, "lb_step_interior before lb_step_boundary");
    DeviceGuard guard(s->p.device);
    return launch_step(s, 1, 1, s->H - 2, write_macro != 0);
}

int lb_step_finish(lb_sim *s)
{
    CPU_UNSUPPORTED(s, "lb_step_finish");
    SCALAR_UNSUPPORTED(s, "lb_step_finish");
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
    SCALAR_UNSUPPORTED(s, "lb_halo_export");
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
    SCALAR_UNSUPPORTED(s, "lb_halo_import");
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
    SCALAR_UNSUPPORTED(s, "lb_halo_floats");
    if (!s) return fail(LB_ERR_ARG, "null handle");
    return HALO_SEGS * s->p.nx;
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
    for (int i = 0; sims && i < count; ++i) SCALAR_UNSUPPORTED(sims[i], "lb_run_group");
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
    for (int i = 0; i < count; ++i)
        if ((rc = ensure_halo_buf(sims[i]))) return rc;
    auto south_nb = [&](int i) { return i > 0 ? i - 1 : (wrap ? count - 1 : -1); };
    auto north_nb = [&](int i) { return i < count - 1 ? i + 1 : (wrap ? 0 : -1); };
    // Halo (table T) of lattice `rel` (0 = current, 1 = the one being written) of every member, on each member's stream `q`: each
    // packs its edge rows into its send buffers once they are complete (`ready`: the member's event that says so; nullptr: the
    // stream's own order does), the receivers scatter them from there into their ghost rows (the kernels of the RCCL path, with the
    // transport replaced by a plain read of the neighbour's buffer)
    auto exchange = [&](hipStream_t lb_sim::*q, const HaloTables &T, int rel, hipEvent_t lb_sim::*ready) -> int {
        const size_t n = (size_t)T.n * sims[0]->p.nx;
        for (int i = 0; i < count; ++i) {
            lb_sim *me = sims[i];
            // my edge rows are complete; my send buffers are free (both neighbours have read the previous halo out of them)
            if (ready) HIP_TRY(hipStreamWaitEvent(me->*q, me->*ready, 0));
            for (int nb : {south_nb(i), north_nb(i)})
                if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->*q, sims[nb]->ev_halo, 0));
            if ((rc = halo_pack(me, me->cur ^ rel, me->*q, T, north_nb(i) >= 0, south_nb(i) >= 0))) return rc;
            HIP_TRY(hipEventRecord(me->ev_packed, me->*q));
        }
        for (int i = 0; i < count; ++i) {
            lb_sim *me = sims[i];
            const int so = south_nb(i), no = north_nb(i);
            for (int nb : {so, no})
                if (nb >= 0) HIP_TRY(hipStreamWaitEvent(me->*q, sims[nb]->ev_packed, 0));
            // my south ghost rows <- what the southern neighbour sent north, and vice versa
            if ((rc = halo_unpack(me, me->cur ^ rel, me->*q, T, so >= 0 ? sims[so]->halo_buf : nullptr,
                                  no >= 0 ? sims[no]->halo_buf + n : nullptr)))
                return rc;
            HIP_TRY(hipEventRecord(me->ev_halo, me->*q));
        }
        return LB_OK;
    };
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipEventRecord(sims[i]->ev_interior, sims[i]->stream));
        HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[i]->ev_interior, 0));
    }
    int hmin = sims[0]->H;
    for (int i = 1; i < count; ++i) hmin = std::min(hmin, sims[i]->H);
    int step_depths = depth_mask(true, true);
    int D = MAX_DEPTH;
    for (int i = 0; i < count; ++i) {
        step_depths &= slab_step_depths(sims[i], hmin);
        D = std::min(D, cycle_depth(sims[i], hmin));
    }
    int left = n_steps;
    if (D && left >= D) {
        const HaloTables &T = cycle_halo(D);
        // The halo cycle of lb_run (full cycles + a lone first half) with the transport replaced: every member packs its edges on its
        // edge stream, the receivers unpack straight from the senders' buffers.
        if ((rc = exchange(&lb_sim::edge_stream, T, 0, nullptr))) return rc;
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
            if ((rc = exchange(&lb_sim::edge_stream, T, 0, nullptr))) return rc;
            DBG_SYNC(2);
            for (int i = 0; i < count; ++i) HIP_TRY(hipStreamWaitEvent(sims[i]->stream, sims[i]->ev_boundary, 0));
        }
        int depth_after = 2 * D;
        if (left >= D) {                            // the lone first half (see run_slab)
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
    // launch by launch, the halo three rows deep, on the communication streams
    if ((rc = exchange(&lb_sim::comm_stream, HALO3, 0, &lb_sim::ev_interior))) return rc;
    DBG_SYNC(2);
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipStreamWaitEvent(sims[i]->stream, sims[i]->ev_halo, 0));
        HIP_TRY(hipStreamWaitEvent(sims[i]->edge_stream, sims[i]->ev_halo, 0));
    }
    while (left > 0) {
        const int adv = next_advance(sims[0], step_depths, left);
        for (int i = 0; i < count; ++i)
            if ((rc = slab_step_launch(sims[i], adv, left == adv))) return rc;
        DBG_SYNC(1);
        if ((rc = exchange(&lb_sim::comm_stream, HALO3, 1, &lb_sim::ev_boundary))) return rc;
        DBG_SYNC(2);
        for (int i = 0; i < count; ++i) {
            if ((rc = slab_step_join(sims[i]))) return rc;
            // a neighbour's next launch overwrites the lattice my comm stream may still be reading
            // from (its old lattice): make every member wait for every halo copy that reads it
            for (int nb : {south_nb(i), north_nb(i)}) {
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
}  // extern "C"
