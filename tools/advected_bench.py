#!/usr/bin/env python3
"""A flow and the scalars it carries: the one-launch step against the launch-per-lattice step, today's sequence and the copy rate.

    python tools/advected_bench.py [--sizes 256,512,1024,2048,4096,8192] [--rounds 3] > profiles/advected_bench.txt

For every box size one periodic flow handle (eager rho, u, v) and two periodic scalar lattices (k_ad_step forced) are created once;
for NS = 1 and NS = 2 four things are timed on those handles IN ALTERNATION, `rounds` times, best of the rounds:
    form 1      lb_run_advected(steps, form = 1): k_fa_step, one launch per step
    form 0      lb_run_advected(steps, form = 0): k_step<MACRO> and one k_ad_step per scalar reading the flow's u, v planes
    sequence    what the existing calls offer for a velocity coupled every step: steps x (lb_run(flow, 1); per scalar
                lb_set_velocity_from and lb_run(scalar, 1)), enqueued without a host wait
    copy        lb_copy_calibration on the flow handle
The first three by a host clock around the enqueue and the wait for every member's stream (the sequence runs on several streams, so
no event pair of one stream brackets it); every member is idle before a sample starts.  `steps` grows as the box shrinks (about
1.3e9 cell steps per sample, 20 ... 2000 steps).  Printed per case: MLUPS of each (cells x steps / time: one step of the whole set
counts once), form 1's compulsory traffic 72 (1 + NS) B x cells x steps / time against the copy rate, each form over the sequence, and
the faster form -- what advected_form (csrc/plan.cpp) is set from.
"""
import argparse
import ctypes as ct
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9 import _native                    # noqa: E402
from LB_D2Q9.simulation import Simulation      # noqa: E402
from LB_D2Q9.variants import K_STEP            # noqa: E402

OMEGAS, GS = (1.6, 1.1), (0.0, 0.01)


def steps_for(n):
    return int(min(2000, max(20, round(1.3e9 / (float(n) * n)))))


def handles(n):
    y = (np.arange(n, dtype=np.float32) + 0.5) / n
    u = np.asfortranarray((0.04 * np.tanh(20. * (y - 0.5)))[None, :] * np.ones((n, 1), np.float32))
    v = np.asfortranarray((0.01 * np.sin(2 * np.pi * y))[:, None] * np.ones((1, n), np.float32))
    flow = Simulation(n, n, 1.7, bc="periodic", eager_macro=True)
    flow.set_fields(np.ones((n, n), np.float32, order="F"), u, v)
    flow.update_feq()
    flow.init_pop()
    dye = np.asfortranarray(np.where((y > 0.3) & (y < 0.6), 0.8, 0.2).astype(np.float32)[None, :] * np.ones((n, 1), np.float32))
    scalars = []
    for om, G in zip(OMEGAS, GS):
        s = Simulation(n, n, om, bc="periodic", semantics="diffusion")
        s.set_reaction(G)
        s.set_variant(K_STEP)
        s.set_fields(dye, u, v)
        s.update_feq()
        s.init_pop()
        scalars.append(s)
    return flow, scalars


def case(n, rounds):
    lib = _native.lib()
    flow, scalars = handles(n)
    hs = (ct.c_void_p * 2)(*[s._h for s in scalars])
    steps = steps_for(n)

    def wait():
        flow.sync()
        for s in scalars:
            s.sync()

    def timed(enqueue):
        wait()
        t0 = time.perf_counter()
        enqueue()
        wait()
        return (time.perf_counter() - t0) * 1e3

    def form(ns, which):
        return timed(lambda: _native.check(lib.lb_run_advected(flow._h, hs, ns, steps, which)))

    def sequence(ns):
        def enqueue():
            for _ in range(steps):
                _native.check(lib.lb_run(flow._h, 1))
                for s in scalars[:ns]:
                    _native.check(lib.lb_set_velocity_from(s._h, flow._h))
                    _native.check(lib.lb_run(s._h, 1))
        return timed(enqueue)

    for ns in (1, 2):
        for f in (form(ns, 1), form(ns, 0), sequence(ns)):      # warm-up
            assert f > 0
        best = {"form1": None, "form0": None, "seq": None}
        copy = 0.
        for _ in range(rounds):
            for k, ms in (("form1", form(ns, 1)), ("form0", form(ns, 0)), ("seq", sequence(ns))):
                best[k] = ms if best[k] is None else min(best[k], ms)
            copy = max(copy, flow.copy_calibration(iters=10)[0])
        upd = float(n) * n * steps
        ml = {k: upd / (ms * 1e-3) / 1e6 for k, ms in best.items()}
        gb = 72. * (1 + ns) * upd / (best["form1"] * 1e-3) / 1e9
        print("n=%5d NS=%d steps=%4d  form 1 %7.0f MLUPS (%5.0f GB/s at %3d B, copy %5.0f GB/s, ratio %.2f)  form 0 %7.0f MLUPS  sequence %7.0f MLUPS  "
              "form 1 / sequence %.2f  form 0 / sequence %.2f  faster form: %d"
              % (n, ns, steps, ml["form1"], gb, 72 * (1 + ns), copy, gb / copy, ml["form0"], ml["seq"], ml["form1"] / ml["seq"],
                 ml["form0"] / ml["seq"], 1 if best["form1"] <= best["form0"] else 0), flush=True)
    for s in [flow] + scalars:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    print("# a flow and NS scalars: lb_run_advected form 1 (k_fa_step, one launch per step) and form 0 (k_step<MACRO> + NS x k_ad_step) against "
          "today's sequence (lb_run(flow, 1) + NS x (lb_set_velocity_from + lb_run(scalar, 1)) per step), host clock around enqueue + wait, best of "
          "%d rounds alternating form 1 / form 0 / sequence / lb_copy_calibration on the same handles; MLUPS = steps of the whole set x cells" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        case(n, a.rounds)


if __name__ == "__main__":
    main()
