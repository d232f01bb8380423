#!/usr/bin/env python3
"""Throughput of k_mf_step (coupled scalar lattices) against the separate k_ad_step launches it replaces and the copy rate.

    python tools/multifield_bench.py [--sizes 1024,4096,8192] [--steps 20] [--rounds 3] > profiles/multifield_bench.txt

For every box size and both families: four LB_SEM_MULTIFIELD handles (periodic / box) and four LB_SEM_DIFFUSION handles
(periodic / open, k_ad_step forced: the single-step kernel a set without coupling would run field by field) are created
once; for NF = 1 ... 4 the engine's timers bracket lb_run_coupled(steps) on the first NF coupled handles, lb_run(steps) on
each of the first NF separate handles (enqueued back to back, timed as one block) and lb_copy_calibration, taken `rounds`
times IN ALTERNATION; best of the rounds.  Printed per case: MLUPS (cell updates of ONE field per second: cells x NF x
steps / time) of both, the coupled launch's compulsory traffic (72 NF + 8) B x cells x steps / time against the copy rate,
and coupled / separate.
"""
import argparse
import ctypes as ct
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9 import _native                    # noqa: E402
from LB_D2Q9.simulation import Simulation      # noqa: E402
from LB_D2Q9.variants import K_STEP            # noqa: E402

OMEGAS, GS = (0.9, 1.3, 1.1, 1.25), (0.02, 0.01, 0.015, 0.005)


def handles(n, sem, bc):
    x = np.arange(n, dtype=np.float32)
    u = np.asfortranarray(0.05 * np.sin(2 * np.pi * x / n)[None, :] * np.ones((n, 1), np.float32))
    v = np.asfortranarray(0.05 * np.cos(2 * np.pi * x / n)[:, None] * np.ones((1, n), np.float32))
    rho = np.full((n, n), 0.2, np.float32, order="F")
    out = []
    for om, G in zip(OMEGAS, GS):
        s = Simulation(n, n, om, bc=bc, semantics=sem)
        s.set_reaction(G)
        s.init_equilibrium(rho, u, v)
        if sem == "diffusion":
            s.set_variant(K_STEP)
        out.append(s)
    return out


def case(n, family, steps, rounds):
    lib = _native.lib()
    mf = handles(n, "multifield", family)
    ad = handles(n, "diffusion", "open" if family == "box" else family)
    hs = (ct.c_void_p * 4)(*[s._h for s in mf])

    def coupled(nf):
        mf[0].timer_start()
        _native.check(lib.lb_run_coupled(hs, nf, steps))
        return mf[0].timer_stop()

    for nf in (1, 2, 3, 4):
        coupled(nf)                             # warm-up
        best_c, best_s, best_copy = None, None, 0.
        for _ in range(rounds):
            ms = coupled(nf)
            best_c = ms if best_c is None else min(best_c, ms)
            t = 0.                              # the separate runs one after the other, each on its own handle's timers
            for s in ad[:nf]:
                t += s.timed_run(steps)
            best_s = t if best_s is None else min(best_s, t)
            gbs, _ = mf[0].copy_calibration(iters=10)
            best_copy = max(best_copy, gbs)
        upd = float(n) * n * steps
        mc, msep = upd * nf / (best_c * 1e-3) / 1e6, upd * nf / (best_s * 1e-3) / 1e6
        gb = (72. * nf + 8.) * upd / (best_c * 1e-3) / 1e9
        print("%-9s n=%5d NF=%d  k_mf_step %7.0f MLUPS (%5.0f GB/s at %3d B, copy %5.0f GB/s, ratio %.2f)  %d x k_ad_step %7.0f MLUPS  "
              "coupled / separate %.2f" % (family, n, nf, mc, gb, 72 * nf + 8, best_copy, gb / best_copy, nf, msep, mc / msep), flush=True)
    for s in mf + ad:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    print("# coupled scalar lattices: k_mf_step (NF fields per launch) against NF separate k_ad_step runs (sum of their times), %d steps per "
          "sample, best of %d rounds alternating coupled / separate / lb_copy_calibration on the same handles; MLUPS = field-cell updates"
          % (a.steps, a.rounds))
    for n in [int(k) for k in a.sizes.split(",")]:
        for family in ("periodic", "box"):
            case(n, family, a.steps, a.rounds)


if __name__ == "__main__":
    main()
