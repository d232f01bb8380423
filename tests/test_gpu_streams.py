"""External streams and device pointers against synchronous twins (tests/stream_scenarios.py has the method and the child scripts).

Everything that can go wrong here is host code deciding WHICH STREAM a kernel or a copy goes on, and none of it shows on the handle's
own stream, where every other test lives.  Each scenario puts a bounded delay on a torch side stream, enqueues the chain under test
behind it without a host wait, synchronises once and compares bit for bit with a twin that waits after every call; a control -- the
handle never told about the stream -- must differ.  Four child processes (torch imported first: one HIP runtime), each run once for
all the scenarios of its group.

MEASURED (MI355X; delay by a torch event pair, the host's enqueue by perf_counter; a scenario fails below a ratio of 4; the delay is
80 ms everywhere -- sized so that the slowest chain met, 2.6 ms, keeps a ratio of 30 -- and capped at 200 ms):
    scenario                                             delay     enqueue        ratio
    split step with a device-side exchange (+ control)   79.9 ms   1.4 - 1.6 ms   51 - 57
    the chain on torch's default stream (a control)      80.0 ms   1.4 ms         58
    graph replay, 3 families x S, S2 (+ controls)        79.6 - 79.9 ms   0.10 - 0.44 ms   181 - 759
    graph capture probe, 3 families                      79.7 - 86.0 ms   1.6 - 1.7 ms   47 - 51
    velocity inlet, three-step passes (+ control)        79.9 ms   0.18 - 0.20 ms 397 - 454
    one-slab peer ring (+ control)                       79.9 ms   1.0 - 1.3 ms   61 - 77
    lb_run_batch (+ control)                             80.0 ms   0.24 - 0.31 ms 257 - 336
    lb_run_coupled / lb_run_fluids                       80.0 ms   0.05 - 0.06 ms 1441 - 1572
    lb_set_force_field, 8 handles x 3 modes              80.0 ms   0.04 - 0.13 ms 621 - 2087
    DistributedSlab.run(9) / run(12), one-rank nccl      79.8 ms   2.1 / 2.6 ms   38 / 30
    timer: behind a delay of 80.0 ms, the handle's interval 20.010 ms around an inner one of 19.998 ms (bound: < inner + 40 ms).
    graph: on S / S2, 160 x run(1) take 0.45 - 0.46 ms to enqueue, run(162) -- ten replays, two launches -- 0.07 - 0.09 ms
    (bound: less than half), so the capture on an external stream succeeds and is what runs.
lb_set_stream's drain and lb_autotune_quick wait on the host by design (no ratio).  Every control differed from its twin.  The
four children take 20 s together.

THE DEFAULT-STREAM HAZARD was real.  DistributedSlab(transport='torch') handed the engine torch's current stream; for the default
stream that handle is 0, which lb_set_stream reads as `own stream`, so kernels and halo copies ran on a stream that nothing ordered
with torch's copies / sends.  With the earlier slabs.py in a one-rank nccl group, 640 x 96, run(9, wait=False): on an idle default
stream 0 of 552960 populations differed from the undivided run (the race went the right way), with 80 ms of other work on the
default stream in front 103680 did (rows 0-8 and 87-95: stale ghosts).  Now the slab runs the exchange on a stream of its own and
hands THAT to the engine (DistributedSlab._torch_buffers), Simulation.use_stream refuses handle 0, and the chain on torch's default stream
is this file's control for that family.

DEFECTS BUILT IN A SCRATCH COPY (never committed), scenarios of this file that turn red (of 14; their child's own case goes with them):
    lb_halo_export on own_stream                                7  (split step, external-stream drain, graph replay, velocity
                                                                   inlet, peer ring, batch, one-rank nccl)
    ensure_graph ignoring graph_stream                          0  not a defect: a hipGraphExec is not bound to the stream it was
                                                                   captured on, hipGraphLaunch(exec, s->stream) decides; the stream in
                                                                   the key only costs a recapture
    coupled_join removed                                        1  (lb_run_coupled; the 143 coupled / fluid / population cases of the
                                                                   existing suite stay green with it)
    the old-stream wait in lb_set_stream removed                2  (both drain scenarios)
    run_slab's final wait of s->stream on ev_halo removed       0  }  these JOINS are not covered, only the forks in front of them
    vel_band_pass's final wait on ev_boundary removed           0  }  (stream_scenarios.py, child FORKS): the tail reads edge rows, which
                                                                   s->stream waits for on ev_boundary inside the run; nothing reads the
                                                                   ghost rows behind ev_halo on s->stream; the band launch is over
                                                                   before the longer interior launch beside it (also at 512 x 128), and
                                                                   no call puts a delay on a handle's edge stream
    lb_set_force_field's device copy with the host-to-device kind   0  the HIP runtime looks the source pointer up and copies device to
                                                                   device whatever the kind says
"""
import os
import subprocess
import sys

import pytest

import stream_scenarios as S

pytestmark = pytest.mark.gpu

_RUNS = {}


def _child(name, tmp_path_factory):
    """Run child `name` once per session; (return code, stdout, stderr)."""
    if name not in _RUNS:
        from conftest import ROOT
        script = tmp_path_factory.mktemp("streams") / ("child_%s.py" % name.lower())
        script.write_text(S.child_source(name))
        # (whatever happens is remembered before anything can raise: a child that hung, or could not be started, is never started
        #  again by the next case that asks for it -- the remaining cases of that child fail from this entry)
        _RUNS[name] = (-1, "", "child %s was started and did not come back" % name)
        text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
        try:
            p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                               capture_output=True, text=True, timeout=300)
            _RUNS[name] = (p.returncode, p.stdout, p.stderr)
        except subprocess.TimeoutExpired as exc:
            _RUNS[name] = (124, text(exc.stdout), text(exc.stderr) + "\nchild %s was ended at its time limit of 300 s" % name)
    return _RUNS[name]


@pytest.mark.parametrize("scenario", sorted(S.SCENARIOS))
def test_scenario(lbhip, tmp_path_factory, scenario):
    """The scenario's line in its child's output: the chain on the external stream equals the waiting twin bit for bit, its control
    differs, every delay outlasted four times the enqueue."""
    rc, out, err = _child(S.SCENARIOS[scenario][0], tmp_path_factory)
    lines = [l for l in out.splitlines() if l.startswith("SCENARIO %s " % scenario)]
    ratios = "\n".join(l for l in out.splitlines() if l.startswith(("RATIO", "TIMER", "GRAPH")))
    assert lines == ["SCENARIO %s OK" % scenario], "\n".join(lines) + "\n" + ratios + "\n" + out[-1500:] + err[-3000:]


@pytest.mark.parametrize("child", sorted(S.CHILDREN))
def test_child_ran_to_its_end(lbhip, tmp_path_factory, child):
    rc, out, err = _child(child, tmp_path_factory)
    print("\n".join(l for l in out.splitlines() if l.startswith(("RATIO", "TIMER", "GRAPH", "SCENARIO"))))
    assert rc == 0 and "%s_OK" % child in out, out[-2000:] + err[-4000:]
