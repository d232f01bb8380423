"""Child scripts of tests/test_gpu_streams.py, and the table of what each scenario covers (test infrastructure; not a test module).

A child is PRELUDE + the bodies of its scenarios + EPILOGUE, written to a file and run by a fresh `python` (torch imported first:
one HIP runtime, which the library then binds to).  Every scenario is a function registered under its name; the child runs them in
order, prints `SCENARIO <name> OK` or `SCENARIO <name> FAIL <why>` for each, and `<CHILD>_OK` when all passed.  A HIP error ends the
child at once (nothing else is started on a device that has reported one).

The method (one shape for every ordering scenario): on a torch side stream S a bounded DELAY (torch.cuda._sleep, sized from a
calibration at the start of the child, capped at 200 ms), behind it -- with no host wait -- the chain under test: the library's
enqueue-only calls and the torch ops that feed or read them on S.  Every device buffer the chain hands over is filled with NaN by a
torch op on S behind the delay.  One synchronisation at the end, then a bitwise comparison with a TWIN that makes the same calls on
its own stream with a host wait after each.  A link that went to another stream runs ahead of the delay and sees poison or
pre-run data.  Each scenario measures the delay (torch event pair) and the host's enqueue time (perf_counter) and fails unless
delay >= 4 x enqueue.  Each family has a CONTROL: the same chain with the handle never told about S, which must DIFFER.
"""

# entry point (or host routine) -> what can go wrong there; the scenario table below must name each at least once
ENTRY_POINTS = ("lb_halo_export", "lb_halo_import", "ensure_graph", "vel_band_pass", "run_slab", "lb_run_batch", "lb_run_coupled",
                "lb_run_fluids", "lb_timer_start", "lb_timer_stop", "lb_autotune_quick", "lb_set_stream", "lb_set_force_field")

# scenario -> (child, the entry points it exercises off the handle's own stream)
SCENARIOS = {
    "split_step_device_exchange": ("FLOW", ("lb_set_stream", "lb_halo_export", "lb_halo_import")),
    "set_stream_drains_own_stream": ("FLOW", ("lb_set_stream",)),
    "set_stream_drains_external_stream": ("FLOW", ("lb_set_stream", "lb_halo_export")),
    "default_stream_cannot_be_named": ("FLOW", ("lb_set_stream", "lb_halo_export", "lb_halo_import")),
    "graph_replay_follows_the_stream": ("FORKS", ("ensure_graph", "lb_set_stream", "lb_halo_export")),
    "velocity_inlet_band_pass": ("FORKS", ("vel_band_pass", "lb_halo_export")),
    "peer_ring_slab_run": ("FORKS", ("run_slab", "lb_halo_export")),
    "timer_on_the_stream": ("FORKS", ("lb_timer_start", "lb_timer_stop")),
    "autotune_quick_on_the_stream": ("FORKS", ("lb_autotune_quick",)),
    "batch_members_on_different_streams": ("SETS", ("lb_run_batch", "lb_halo_export")),
    "coupled_members_on_different_streams": ("SETS", ("lb_run_coupled",)),
    "fluids_on_one_external_stream": ("SETS", ("lb_run_fluids",)),
    "force_field_from_device_pointers": ("SETS", ("lb_set_force_field", "lb_set_stream")),
    "one_rank_nccl_torch_transport": ("NCCL", ("lb_set_stream", "lb_halo_export", "lb_halo_import")),
}

PRELUDE = r'''
import os
import sys
import time
# (the handles of a scenario and torch's side streams must not share a hardware queue: streams that share one run in submission
#  order, and a control would then wait behind the delay like everything else.  Read when the HIP runtime loads, i.e. at import torch.
#  For the same reason a child makes its side streams ONCE, below: every torch.cuda.Stream() is another stream of torch's pool,
#  each keeps the queue it first ran on, and the sixteenth made in one process shared its queue with a handle's own stream.)
os.environ["GPU_MAX_HW_QUEUES"] = "24"
import torch                                    # first: ONE HIP runtime in the process, torch's; the library binds to it
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import ctypes as ct
from LB_D2Q9 import _native
from LB_D2Q9 import variants as V
from LB_D2Q9.simulation import Simulation

torch.cuda.set_device(0)
DEV = torch.device("cuda", 0)
L = _native.lib()
W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
FLOW = ("f", "rho", "u", "v")
DELAY_MS, DELAY_CAP_MS, MIN_RATIO = 80., 200., 4.


def _calibrate():
    """torch.cuda._sleep cycles per millisecond on this device (the clock it spins on is the device's business)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000000)                  # (the first launch loads the kernel)
    torch.cuda.synchronize()
    n = 20000000
    e0.record()
    torch.cuda._sleep(n)
    e1.record()
    torch.cuda.synchronize()
    return n / e0.elapsed_time(e1)


CYCLES_PER_MS = _calibrate()
SIDE = [torch.cuda.Stream(DEV) for _ in range(2)]      # the side streams of every scenario of this child
assert all(s_.cuda_stream != 0 for s_ in SIDE)


class Delay(object):
    """A bounded delay on `stream`, bracketed by a torch event pair; the host's enqueue of the chain runs from here to done()."""

    def __init__(self, stream, ms=DELAY_MS):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.e0.record()
            torch.cuda._sleep(int(min(ms, DELAY_CAP_MS) * CYCLES_PER_MS))
            self.e1.record()
        self.t0 = self.t1 = time.perf_counter()

    def done(self):
        self.t1 = time.perf_counter()

    def check(self, what):
        """After the final synchronisation: the scenario proves something only if the delay outlasted the enqueue."""
        delay, enq = self.e0.elapsed_time(self.e1), (self.t1 - self.t0) * 1e3
        print("RATIO %s delay %.1f ms enqueue %.2f ms ratio %.0f" % (what, delay, enq, delay / max(enq, 1e-3)), flush=True)
        assert delay >= MIN_RATIO * enq, "%s: the delay (%.1f ms) did not outlast 4 x the enqueue (%.2f ms)" % (what, delay, enq)
        assert delay <= 1.5 * DELAY_CAP_MS, "%s: delay %.1f ms" % (what, delay)


def noisy(nx, ny, seed, amp=0.02):
    rng = np.random.default_rng(seed)
    return (W[None, None, :] * (1 + amp * rng.standard_normal((nx, ny, 9)))).astype(np.float32)


def nan_buf(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def differing(a, b):
    """Names of the arrays of two dicts that are not bit for bit the same."""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    return [k for k in sorted(a) if not np.array_equal(a[k], b[k])]


def assert_same(a, b, what):
    d = differing(a, b)
    assert not d, "%s: %s differ from the waiting twin (%s)" % (what, d, ", ".join(
        "%s: %d cells, %d NaN" % (k, int((a[k] != b[k]).sum()), int(np.isnan(a[k]).sum())) for k in d))


def assert_control_differs(a, b, what):
    assert differing(a, b), "%s: the control, never told about the stream, equals the twin: the scenario cannot see a mis-ordered link" % what


def export_clone(sim, stream, buf, side=1):
    """The chain's tail: NaN into the buffer by a torch op on `stream`, the edge rows exported over it, a clone on `stream`."""
    with torch.cuda.stream(stream):
        buf.fill_(float("nan"))
        sim.halo_export(side, buf.data_ptr())
        return buf.clone()


def export_waiting(sim, side=1):
    sim.sync()
    out = np.zeros(sim.halo_floats(), np.float32)
    sim.halo_export(side, out)
    sim.sync()
    return out


def handles(sims):
    return (ct.c_void_p * len(sims))(*[s._h for s in sims])


SCENARIOS = []


def scenario(fn):
    SCENARIOS.append(fn)
    return fn
'''

EPILOGUE = r'''
failed = []
for fn in SCENARIOS:
    try:
        fn()
        torch.cuda.synchronize()
        print("SCENARIO %s OK" % fn.__name__, flush=True)
    except AssertionError as exc:
        torch.cuda.synchronize()
        failed.append(fn.__name__)
        print("SCENARIO %s FAIL %s" % (fn.__name__, str(exc).replace("\n", " ")), flush=True)
    except Exception:                           # (a HIP error among them: nothing more is started on this device)
        import traceback
        traceback.print_exc()
        print("SCENARIO %s ERROR" % fn.__name__, flush=True)
        sys.exit(3)
if failed:
    sys.exit("failed: %s" % failed)
print("%s_OK" % CHILD)
'''

# ---- child FLOW: the split step, lb_set_stream's drain, the stream the slabs hand to the engine ------------------------------------
FLOW = r'''
CHILD = "FLOW"
NX, NY, OMEGA, STEPS = 640, 96, 1.35, 6           # the shape of test_distributed_checkpoint_on_the_real_engine_single_rank


def split_case():
    rng = np.random.default_rng(11)
    f0 = noisy(NX, NY, 11)
    mask = rng.random((NX, NY)) < 0.03
    return f0, mask


def split_chain(sim, stream, bufs, steps):
    """What DistributedSlab.run makes of n steps on one periodic rank, by hand: every library call enqueue-only, the torch copies on
    `stream`.  The ghosts first (the handle has none yet), then per step boundary, interior, export, copies, import, finish."""
    send_s, send_n, recv_s, recv_n = bufs

    def exchange():
        sim.halo_export(0, send_s.data_ptr())
        sim.halo_export(1, send_n.data_ptr())
        with torch.cuda.stream(stream):
            recv_s.copy_(send_n)
            recv_n.copy_(send_s)
        sim.halo_import(0, recv_s.data_ptr())
        sim.halo_import(1, recv_n.data_ptr())

    with torch.cuda.stream(stream):
        for b in bufs:
            b.fill_(float("nan"))
    exchange()
    for it in range(steps):
        sim.step_boundary(it == steps - 1)
        sim.step_interior(it == steps - 1)
        exchange()
        sim.step_finish()


def undivided(f0, mask, steps):
    one = Simulation(NX, NY, OMEGA, bc="periodic", obstacle_mask=mask)
    one.set_f(f0)
    one.run(steps)
    want = one.get_fields(FLOW)
    one.close()
    return want


def split_run(f0, mask, stream, tell, what):
    """tell: the stream handle given to use_stream (None: the handle is never told -- the control)."""
    sim = Simulation(NX, NY, OMEGA, bc="periodic", obstacle_mask=mask, halo=True)
    sim.set_f(f0)
    if tell is not None:
        sim.use_stream(tell)
    bufs = [nan_buf(sim.halo_floats()) for _ in range(4)]
    torch.cuda.synchronize()
    d = Delay(stream)
    split_chain(sim, stream, bufs, STEPS)
    d.done()
    torch.cuda.synchronize()
    d.check(what)
    got = sim.get_fields(FLOW)
    sim.use_stream(None)
    sim.close()
    return got


@scenario
def split_step_device_exchange():
    f0, mask = split_case()
    want = undivided(f0, mask, STEPS)
    S = SIDE[0]
    assert S.cuda_stream != 0
    assert_same(split_run(f0, mask, S, S.cuda_stream, "split step on S"), want, "split step on S")
    assert_control_differs(split_run(f0, mask, S, None, "split step, control"), want, "split step")


@scenario
def default_stream_cannot_be_named():
    """What DistributedSlab's torch-driven exchange did until this file found it out: the chain of the split step with torch's current
    DEFAULT stream.  Its handle is 0, which lb_set_stream reads as `back to the own stream`, so it cannot be handed over:
    Simulation.use_stream(0) refuses.  The delay and the copies on the default stream, the engine on its own: the imports read
    buffers the copies have not filled, and the result differs from the undivided run -- this family's control.  (What the slab does
    now -- a torch stream of its own, handed to the engine -- is the split step above by hand and the NCCL child end to end.)"""
    f0, mask = split_case()
    want = undivided(f0, mask, STEPS)
    default = torch.cuda.current_stream()
    assert default.cuda_stream == 0                 # (torch's default stream is the legacy null stream)
    try:
        Simulation(64, 64, 1.2, bc="periodic").use_stream(default.cuda_stream)
        raise AssertionError("use_stream(0) was accepted: the default stream cannot be named, NULL means the own stream")
    except ValueError:
        pass
    assert_control_differs(split_run(f0, mask, default, None, "default stream, control"), want, "default stream")


@scenario
def set_stream_drains_own_stream():
    nx, ny = 1024, 160
    rng = np.random.default_rng(21)
    f0, mask = noisy(nx, ny, 21), rng.random((nx, ny)) < 0.02
    twin = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    twin.set_f(f0)
    twin.run(57)
    want = twin.get_fields(FLOW)
    twin.close()
    S = SIDE[0]
    sim = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    sim.set_f(f0)
    sim.run(50, wait=False)                        # on the own stream
    sim.use_stream(S.cuda_stream)
    sim.run(7, wait=False)
    torch.cuda.synchronize()
    assert_same(sim.get_fields(FLOW), want, "run(50) on the own stream, run(7) on S")
    sim.use_stream(None)
    sim.close()


@scenario
def set_stream_drains_external_stream():
    """The same with the OLD stream an external one, so that a delay can hold its work back: run(50) and an export wait on S0 behind
    the delay, use_stream(S) must drain S0 before a clone of the exported rows and run(7) follow on S.  (The drain is a host wait
    by design: no delay / enqueue ratio here.)  Control: never told about S -- the clone on S then reads the poison."""
    nx, ny = 1024, 160
    rng = np.random.default_rng(22)
    f0, mask = noisy(nx, ny, 22), rng.random((nx, ny)) < 0.02
    twin = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    twin.set_f(f0)
    twin.run(50)
    rows = export_waiting(twin)
    twin.run(7)
    want = dict(twin.get_fields(FLOW), rows=rows)
    twin.close()
    for told in (True, False):
        S0, S = SIDE[0], SIDE[1]
        sim = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
        sim.set_f(f0)
        sim.use_stream(S0.cuda_stream)
        buf = nan_buf(sim.halo_floats())
        torch.cuda.synchronize()
        Delay(S0)
        sim.run(50, wait=False)
        sim.halo_export(1, buf.data_ptr())
        if told:
            sim.use_stream(S.cuda_stream)
        with torch.cuda.stream(S):
            got_rows = buf.clone()
        sim.run(7, wait=False)
        torch.cuda.synchronize()
        got = dict(sim.get_fields(FLOW), rows=got_rows.cpu().numpy())
        sim.use_stream(None)
        sim.close()
        if told:
            assert_same(got, want, "run(50) on S0, run(7) on S")
        else:
            assert_control_differs(got, want, "lb_set_stream's drain")
'''

# ---- child FORKS: graph replay, the forks from s->stream to edge_stream / comm_stream, timer and tuner --------------------------------
# Of vel_band_pass and run_slab only the FORK side is tested: that the band / edge / exchange launches wait for what s->stream holds
# (the delay) and that the run and its tail follow s->stream.  The JOINS at their ends -- s->stream waiting on ev_boundary for the
# bands, on ev_halo for the last exchange -- are not: the tail reads edge rows only, which s->stream already waits for on ev_boundary
# inside the run, nothing reads the ghost rows that ev_halo guards on s->stream before the device-wide synchronisation (a by-hand
# step_boundary behind a peer run would, but the launch it has to wait for is over long before the interior launch in front of it),
# and no call from outside puts a delay on a handle's edge stream.  Both waits removed in a scratch build turn nothing red here.
FORKS = r'''
CHILD = "FORKS"


def flow_chain(sim, stream, tell, n, buf, old=None):
    """use_stream, delay (on `old` as well: a launch that went to the stream the handle has just left is held back there),
    run(n, wait=False), export over the poison, clone; all on `stream`, no host wait after the switch."""
    sim.use_stream(tell)
    torch.cuda.synchronize()
    if old is not None:
        Delay(old)
    d = Delay(stream)
    sim.run(n, wait=False)
    rows = export_clone(sim, stream, buf)
    d.done()
    return d, rows


def replay_is_cheaper_than_launches(sim, stream, what):
    """That a graph IS captured and replayed on the external stream (a capture that fails there is no error: the run falls back to
    single launches, with the same bits): behind a delay, so that only the host's enqueue is timed, 160 steps as lb_run(h, 1) x 160
    -- which never replays -- against lb_run(h, 162): ten replays and two launches (even counts: the lattice parity the capture is
    keyed by stays).  Twelve enqueues against 160 launches of the same kernel: were the second a fall-back to 162 launches, it
    could not take less than half the time of the first (the ctypes calls the first adds cost a fraction of a launch each).  The
    best of three, each way."""
    sim.use_stream(stream.cuda_stream)
    sim.run(18, wait=False)                         # (the capture itself is not timed)
    torch.cuda.synchronize()
    d = Delay(stream)
    eager, replay = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(160):
            L.lb_run(sim._h, 1)
        t1 = time.perf_counter()
        L.lb_run(sim._h, 162)
        t2 = time.perf_counter()
        eager.append(t1 - t0)
        replay.append(t2 - t1)
    d.done()
    torch.cuda.synchronize()
    d.check("graph capture %s" % what)
    print("GRAPH %s 160 x run(1) %.3f ms, run(162) %.3f ms" % (what, min(eager) * 1e3, min(replay) * 1e3), flush=True)
    assert min(replay) < 0.5 * min(eager), "%s: run(162) took %.3f ms to enqueue, 160 x run(1) %.3f ms: no graph is replayed on this stream" % (
        what, min(replay) * 1e3, min(eager) * 1e3)


@scenario
def graph_replay_follows_the_stream():
    """64 x 64, pinned to the single-step kernel: run(40) replays the 16-launch graph twice and steps 8 times.  On S, then on S2 (the
    handle recaptures; the delay is on S as well, where a replay of the old capture would go), then on the own stream again (delay
    on S2).  The twin steps run(1) at a time and never replays.  First, that there is a replay on S and on S2 at all."""
    for i, bc in enumerate(("pipe", "periodic", "cavity")):
        probe = Simulation(64, 64, 1.4, bc=bc, inlet_rho=1.004, lid_u=0.05)
        probe.set_variant(V.K_STEP)
        probe.set_f(noisy(64, 64, 30))
        replay_is_cheaper_than_launches(probe, SIDE[i % 2], "%s on S%s" % (bc, "2" if i % 2 else ""))
        probe.use_stream(None)
        probe.close()
        nx = ny = 64
        rng = np.random.default_rng(31)
        f0, mask = noisy(nx, ny, 31), np.zeros((nx, ny), bool)
        mask[20:24, 30:37] = True
        kw = dict(bc=bc, obstacle_mask=mask, inlet_rho=1.004, lid_u=0.05)
        twin = Simulation(nx, ny, 1.4, **kw)
        twin.set_variant(V.K_STEP)
        twin.set_f(f0)
        want = {}
        for seg in range(3):
            for _ in range(40):
                twin.run(1)
            want["rows%d" % seg] = export_waiting(twin)
        want.update(twin.get_fields(FLOW))
        twin.close()
        for told in (True, False):
            S, S2 = SIDE[0], SIDE[1]
            sim = Simulation(nx, ny, 1.4, **kw)
            sim.set_variant(V.K_STEP)
            sim.set_f(f0)
            buf = nan_buf(sim.halo_floats())
            got = {}
            d1, got["rows0"] = flow_chain(sim, S, S.cuda_stream if told else None, 40, buf)
            d2, got["rows1"] = flow_chain(sim, S2, S2.cuda_stream if told else None, 40, buf, old=S)
            sim.use_stream(None)
            torch.cuda.synchronize()
            Delay(S2)
            sim.run(40, wait=False)
            torch.cuda.synchronize()
            got["rows2"] = export_waiting(sim)
            d1.check("graph replay %s on S%s" % (bc, "" if told else ", control"))
            d2.check("graph replay %s on S2%s" % (bc, "" if told else ", control"))
            got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
            got.update(sim.get_fields(FLOW))
            sim.close()
            if told:
                assert_same(got, want, "graph replay, %s" % bc)
            else:
                assert_control_differs(got, want, "graph replay, %s" % bc)


def forked_run(make, n, what):
    """delay, run(n, wait=False), export, clone on S against the waiting twin; the control never told about S."""
    twin = make()
    twin.run(n)
    want = dict(twin.get_fields(FLOW), rows=export_waiting(twin))
    twin.close()
    for told in (True, False):
        S = SIDE[0]
        sim = make()
        buf = nan_buf(sim.halo_floats())
        d, rows = flow_chain(sim, S, S.cuda_stream if told else None, n, buf)
        torch.cuda.synchronize()
        d.check(what + ("" if told else ", control"))
        got = dict(sim.get_fields(FLOW), rows=rows.cpu().numpy())
        sim.use_stream(None)
        sim.close()
        if told:
            assert_same(got, want, what)
        else:
            assert_control_differs(got, want, what)


@scenario
def velocity_inlet_band_pass():
    nx, ny = 1024, 160
    rng = np.random.default_rng(41)
    f0, mask = noisy(nx, ny, 41), rng.random((nx, ny)) < 0.02
    mask[:2, :] = mask[-2:, :] = False
    mask[:, :2] = mask[:, -2:] = False

    def make():
        s = Simulation(nx, ny, 1.5, bc="velocity_inlet", inlet_u=0.03, obstacle_mask=mask)
        s.set_variant(V.K_STEP3)
        assert s.steps_per_launch() == 3, s.hot_kernel()
        s.set_f(f0)
        return s
    forked_run(make, 10, "velocity inlet, three-step passes")       # 3 + 3 + 3 band passes and a single step (or 1 + 3 x 3)


@scenario
def peer_ring_slab_run():
    nx, ny = 1024, 160                                # the height of test_peer_transport_self_ring_equals_plain_run
    rng = np.random.default_rng(42)
    f0, mask = noisy(nx, ny, 42), rng.random((nx, ny)) < 0.02

    def make():
        ring = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask, halo=True)
        rows = ring.MASK_HALO_ROWS
        ring.set_obstacle_mask_halo(mask[:, -rows:].T.copy(), mask[:, :rows].T.copy())
        desc = ring.peer_export()
        ring.peer_connect(0, 1, desc, desc, ny)
        ring.set_f(f0)
        return ring
    forked_run(make, 33, "one-slab peer ring")        # cycles, a lone first half and launch-by-launch steps
    plain = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    plain.set_f(f0)
    plain.run(33)
    ring = make()
    ring.run(33)
    assert_same(ring.get_fields(FLOW), plain.get_fields(FLOW), "the ring against the plain handle")
    ring.close()
    plain.close()


@scenario
def timer_on_the_stream():
    """timer_start behind a delay on S, then an interval bracketed by a torch event pair, then timer_stop: the handle's interval
    holds the inner one (one stream, one clock) and not the delay in front of its start -- a start event recorded on the own stream
    would be taken at once and the interval would hold the whole delay."""
    S = SIDE[0]
    sim = Simulation(256, 128, 1.3, bc="periodic")
    sim.set_f(noisy(256, 128, 51))
    sim.use_stream(S.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    d = Delay(S)
    with torch.cuda.stream(S):
        sim.timer_start()
        e0.record()
        torch.cuda._sleep(int(20. * CYCLES_PER_MS))
        e1.record()
        d.done()
        ms = sim.timer_stop()
    inner, delay = e0.elapsed_time(e1), d.e0.elapsed_time(d.e1)
    d.check("timer")
    print("TIMER handle %.3f ms inner %.3f ms delay in front %.1f ms" % (ms, inner, delay), flush=True)
    assert inner >= 10., inner
    assert ms >= inner, "the handle's interval (%.3f ms) is shorter than one inside it on the same stream (%.3f ms)" % (ms, inner)
    assert ms < inner + delay / 2, "the handle's interval (%.3f ms) holds the delay in front of timer_start (%.1f ms; inner %.3f ms)" % (ms, delay, inner)
    sim.use_stream(None)
    sim.close()


@scenario
def autotune_quick_on_the_stream():
    nx, ny = 1024, 160
    rng = np.random.default_rng(52)
    f0, mask = noisy(nx, ny, 52), rng.random((nx, ny)) < 0.02
    S = SIDE[0]
    sim = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    sim.set_f(f0)
    sim.use_stream(S.cuda_stream)
    Delay(S, 20.)
    used = L.lb_autotune_quick(sim._h, 4000)
    assert used > 0, "lb_autotune_quick did nothing (%d)" % used
    sim.run(5, wait=False)
    torch.cuda.synchronize()
    got = sim.get_fields(FLOW)
    sim.use_stream(None)
    sim.close()
    twin = Simulation(nx, ny, 1.6, bc="periodic", obstacle_mask=mask)
    twin.set_variant(V.K_STEP)
    twin.set_f(f0)
    twin.run(used + 5)
    assert_same(got, twin.get_fields(FLOW), "lb_autotune_quick on S (%d steps)" % used)
    twin.close()
'''

# ---- child SETS: members on different streams, device pointers --------------------------------------------------------------------------
SETS = r'''
CHILD = "SETS"


@scenario
def batch_members_on_different_streams():
    """Three periodic 96 x 64 handles; member 1 on S with a delayed run(3) of its own pending, lb_run_batch on member 0's own stream
    (the join), member 1 alone on S again (the release), its edge rows exported over the poison and cloned on S."""
    nx, ny, omegas = 96, 64, (1.1, 1.4, 1.7)
    f0 = [noisy(nx, ny, 60 + i) for i in range(3)]

    def make():
        ms = [Simulation(nx, ny, om, bc="periodic") for om in omegas]
        for m, f in zip(ms, f0):
            m.set_f(f)
        return ms

    def fields(ms, rows):
        out = {"rows": rows}
        for i, m in enumerate(ms):
            for k, a in m.get_fields(FLOW).items():
                out["m%d_%s" % (i, k)] = a
        return out

    tw = make()
    tw[1].run(3)
    _native.check(L.lb_run_batch(handles(tw), 3, 4))
    for m in tw:
        m.sync()
    tw[1].run(2)
    want = fields(tw, export_waiting(tw[1]))
    for m in tw:
        m.close()
    for told in (True, False):
        S = SIDE[0]
        ms = make()
        if told:
            ms[1].use_stream(S.cuda_stream)
        buf = nan_buf(ms[1].halo_floats())
        torch.cuda.synchronize()
        d = Delay(S)
        ms[1].run(3, wait=False)
        _native.check(L.lb_run_batch(handles(ms), 3, 4))
        ms[1].run(2, wait=False)
        rows = export_clone(ms[1], S, buf)
        d.done()
        torch.cuda.synchronize()
        d.check("lb_run_batch" + ("" if told else ", control"))
        got = fields(ms, rows.cpu().numpy())
        ms[1].use_stream(None)
        for m in ms:
            m.close()
        if told:
            assert_same(got, want, "lb_run_batch, member 1 on S")
        else:
            assert_control_differs(got, want, "lb_run_batch")


@scenario
def coupled_members_on_different_streams():
    """Two multifield 37 x 23 handles, member 1 on S with a delayed run(3) pending; lb_run_coupled on member 0's own stream; member 1
    alone on S again.  (The family's control is the batch's: these handles take no device buffer a torch op could poison.)"""
    nx, ny = 37, 23
    rng = np.random.default_rng(70)
    f0 = [(0.3 * noisy(nx, ny, 70 + i, 0.1)).astype(np.float32) for i in range(2)]
    u, v = (0.05 * rng.standard_normal((2, nx, ny))).astype(np.float32)

    def make():
        ms = [Simulation(nx, ny, om, bc="box", semantics="multifield") for om in (1.2, 1.5)]
        for m, f, g in zip(ms, f0, (0.05, 0.02)):
            m.set_reaction(g)
            m.set_fields(np.ones((nx, ny), np.float32), u, v)
            m.set_f(f)
        return ms

    def fields(ms):
        return {"m%d_%s" % (i, k): a for i, m in enumerate(ms) for k, a in m.get_fields(("f", "rho")).items()}

    tw = make()
    tw[1].run(3)
    _native.check(L.lb_run_coupled(handles(tw), 2, 4))
    for m in tw:
        m.sync()
    tw[1].run(2)
    want = fields(tw)
    for m in tw:
        m.close()
    S = SIDE[0]
    ms = make()
    ms[1].use_stream(S.cuda_stream)
    torch.cuda.synchronize()
    d = Delay(S)
    ms[1].run(3, wait=False)
    _native.check(L.lb_run_coupled(handles(ms), 2, 4))
    ms[1].run(2, wait=False)
    d.done()
    torch.cuda.synchronize()
    d.check("lb_run_coupled")
    got = fields(ms)
    ms[1].use_stream(None)
    for m in ms:
        m.close()
    assert_same(got, want, "lb_run_coupled, member 1 on S")


@scenario
def fluids_on_one_external_stream():
    from LB_D2Q9.coupled import Shan_Chen_Fluids
    nx, ny = 21, 13
    f0 = np.stack([noisy(nx, ny, 80 + i, 0.05) * (0.5 + 0.25 * i) for i in range(3)], axis=2).astype(np.float32)
    keys = ("f", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary")

    def make():
        fl = Shan_Chen_Fluids(nx, ny, (1.0, 1.3, 1.6), bc="periodic")
        fl.set_interactions([(0, 1, 0.2, "linear", 0.), (1, 2, 0.15, "shan_chen", 0.8), (0, 0, -0.1, "shan_chen", 1.)])
        fl.set_body_force(0, 1e-4, 0.)
        fl.set_f(np.asfortranarray(f0))
        return fl

    tw = make()
    for n in (3, 4, 2):
        tw.run(n)
    want = tw.get_fields(keys)
    tw.close()
    S = SIDE[0]
    fl = make()
    for m in fl.members:
        m.use_stream(S.cuda_stream)
    torch.cuda.synchronize()
    d = Delay(S)
    for n in (3, 4, 2):
        fl.run(n, wait=False)
    d.done()
    torch.cuda.synchronize()
    d.check("lb_run_fluids")
    got = fl.get_fields(keys)
    for m in fl.members:
        m.use_stream(None)
    fl.close()
    assert_same(got, want, "lb_run_fluids, all members on S")


@scenario
def force_field_from_device_pointers():
    """lb_set_force_field(h, gx, gy, 1) with torch tensors against the same planes from numpy: the total force of the last step and
    five steps of f, bit for bit; dropped and set again.  The tensors are written on S behind a delay.  The copy is ordered on the
    handle's stream: a handle on its own stream owes a wait on S (the control, without it, copies the poison; with it, it is the
    numpy handle again) -- these two modes carry the contract.  A handle on S owes none, but that mode cannot tell which stream
    the copy went on: lb_set_force_field first drains the handle's stream, S and the writes on it included, before it enqueues
    anything; it shows that the call is usable from there and gives the same bits."""
    keys = ("f", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary")
    for sem in ("porous", "multifluid"):
        for nx, ny in ((37, 23), (261, 9)):
            for bc in ("periodic", "zero_gradient"):
                what = "%s %dx%d %s" % (sem, nx, ny, bc)
                rng = np.random.default_rng([nx, ny, len(sem), len(bc)])
                f0 = noisy(nx, ny, 90, 0.05)
                gx, gy = (1e-3 * rng.standard_normal((2, nx, ny))).astype(np.float32)
                hx, hy = (1e-3 * rng.standard_normal((2, nx, ny))).astype(np.float32)

                def make():
                    s = Simulation(nx, ny, 1.3, bc=bc, semantics=sem)
                    if sem == "porous":
                        s.set_porous(0.8, 0.1, 5., 0.2)
                    else:
                        s.set_interactions([(0, 0, _native.LB_PSI_SHAN_CHEN, 0 if bc == "periodic" else 1, -0.1, 1.)])
                    s.set_body_force(1e-4, -2e-4)
                    s.set_f(f0)
                    assert s.layout()["pitch"] != nx, s.layout()
                    return s

                def dense(a):
                    return torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)          # [ny][nx], x fastest: the ABI's layout

                a = make()
                a.set_force_field(gx, gy)
                a.run(5)
                want1 = a.get_fields(keys)
                a.set_force_field(None, None)
                a.run(2)
                a.set_force_field(hx, hy)
                a.run(5)
                want2 = a.get_fields(keys)
                a.close()
                src = [dense(x) for x in (gx, gy, hx, hy)]
                for mode in ("on S", "own stream, waits for S", "control"):
                    S = SIDE[0]
                    b = make()
                    if mode == "on S":
                        b.use_stream(S.cuda_stream)
                    t = [nan_buf(nx * ny) for _ in range(4)]
                    torch.cuda.synchronize()
                    d = Delay(S)
                    with torch.cuda.stream(S):
                        for dst, s_ in zip(t, src):
                            dst.copy_(s_.reshape(-1))
                    d.done()                            # (the two modes that wait do so by design: lb_set_force_field drains the handle's stream first)
                    if mode == "own stream, waits for S":
                        S.synchronize()
                    _native.check(L.lb_set_force_field(b._h, t[0].data_ptr(), t[1].data_ptr(), 1))
                    b.run(5, wait=False)
                    if mode == "control":
                        d.done()                        # the copy the control makes must have run inside the delay
                    torch.cuda.synchronize()
                    d.check("lb_set_force_field %s, %s" % (what, mode))
                    got1 = b.get_fields(keys)
                    _native.check(L.lb_set_force_field(b._h, None, None, 0))
                    b.run(2)
                    _native.check(L.lb_set_force_field(b._h, t[2].data_ptr(), t[3].data_ptr(), 1))
                    b.run(5)
                    got2 = b.get_fields(keys)
                    b.use_stream(None)
                    b.close()
                    if mode == "control":
                        assert_control_differs(got1, want1, "lb_set_force_field %s" % what)
                    else:
                        assert_same(got1, want1, "lb_set_force_field %s, %s" % (what, mode))
                        assert_same(got2, want2, "lb_set_force_field %s, %s, dropped and set again" % (what, mode))
'''

# ---- child NCCL: the torch-driven transport end to end, one rank ----------------------------------------------------------------------
NCCL = r'''
CHILD = "NCCL"


@scenario
def one_rank_nccl_torch_transport():
    """DistributedSlab(transport='torch') in a one-rank nccl group: 9 steps, a checkpoint, 12 more, against the undivided run(21).  A
    delay sits on the slab's exchange stream in front of each run, which only enqueues (wait=False)."""
    import socket
    import tempfile
    import torch.distributed as dist
    from LB_D2Q9.slabs import DistributedSlab
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        nx, ny = 640, 96
        rng = np.random.default_rng(11)
        f0 = noisy(nx, ny, 11)
        mask = rng.random((nx, ny)) < 0.03
        one = Simulation(nx, ny, 1.35, bc="periodic", obstacle_mask=mask)
        one.set_f(f0)
        one.run(21)
        want = one.get_fields(FLOW)
        one.close()
        a = DistributedSlab(nx, ny, 1.35, bc="periodic", obstacle_mask=mask, transport="torch", device=0)
        a.set_f(f0)
        S = a.exchange_stream()
        assert S is not None and S.cuda_stream != 0
        torch.cuda.synchronize()
        d = Delay(S)
        a.run(9, wait=False)
        d.done()
        torch.cuda.synchronize()
        d.check("DistributedSlab.run(9)")
        with tempfile.TemporaryDirectory() as tmp:
            a.save_checkpoint(os.path.join(tmp, "ck"))
            b = DistributedSlab.from_checkpoint(os.path.join(tmp, "ck"), transport="torch", device=0)
        S = b.exchange_stream()
        torch.cuda.synchronize()
        d = Delay(S)
        b.run(12, wait=False)
        d.done()
        torch.cuda.synchronize()
        d.check("DistributedSlab.run(12)")
        assert_same(b.get_local_fields(FLOW), want, "one-rank nccl group, transport='torch'")
    finally:
        dist.destroy_process_group()
'''

CHILDREN = {"FLOW": FLOW, "FORKS": FORKS, "SETS": SETS, "NCCL": NCCL}


def child_source(name):
    return PRELUDE + CHILDREN[name] + EPILOGUE
