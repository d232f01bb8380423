#!/usr/bin/env python3
"""Per-wave timeline of one k_step4 / k_deep launch (diagnostic build, LB_DIAG bit 12): when each wave started and ended, on which
XCD / CU / SIMD.  Usage (GPU box): [LB_TIMELINE_BC=pipe] [LB_TIMELINE_DEPTH=6|7] python tools/wave_timeline.py [n]

k_deep2<7> (four waves per item): LB_TIMELINE_DEEP2=1 LB_TIMELINE_DEPTH=7; the report adds, per CU with two workgroups, when each ended,
and what shares a SIMD.  Its issue-priority mode (csrc/kernels_deep2.h: deep2_set_prio; 0 none, 1 front waves, 2 back waves) is chosen
per run by LB_DIAG bits 25-26 of the diagnostic build: LB_DIAG = 4096 | ((mode + 1) << 25), i.e. 33558528 / 67112960 / 100667392 for
modes 0 / 1 / 2; plain 4096 runs the mode the library launches with.  (profiles/deep2_priority_ab.txt)
Which body a wave enters (deep2_take_role): + 134217728 (bit 27) = the static roles (by the wave's number) instead of roles by SIMD;
+ (s << 28), s = 2 / 3 = another flip signal (wave-slot parity / LDS half) than the launch-order bit.  (profiles/deep2_roles_ab.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "2d-lb_amd"), ROOT]
os.environ["LB_LIB"] = os.environ.get("LB_TIMELINE_LIB") or os.path.join(ROOT, "2d-lb_amd", "LB_D2Q9", "liblbhip_diag.so")
os.environ["LB_DIAG"] = os.environ.get("LB_DIAG", "4096")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    ny = int(os.environ.get("LB_TIMELINE_NY", n))
    from LB_D2Q9.simulation import Simulation
    from LB_D2Q9.variants import DEEP2, marching
    from bench import shear_layer
    # (the records travel in the rho array: no launch stores rho, u, v on this handle, and LB_DIAG bit 12 keeps lb_get_macro
    #  from rebuilding them)
    sim = Simulation(n, ny, 1.7, bc=os.environ.get("LB_TIMELINE_BC", "periodic"), inlet_rho=1.0005)
    depth = int(os.environ.get("LB_TIMELINE_DEPTH", "4"))
    deep2 = os.environ.get("LB_TIMELINE_DEEP2") == "1"             # k_deep2<7>: four waves per item (front / back x down / up)
    assert depth in (4, 6, 7), depth
    sim.set_variant(marching(depth) | (DEEP2 if deep2 else 0))
    sim.init_equilibrium(*shear_layer(n, ny, 0, ny))
    sim.run(2 * depth)
    sim.run(depth)                                # the launch whose timeline is read
    raw = sim.get_fields(("rho",))["rho"]
    u = np.ascontiguousarray(raw.T).view(np.uint32).reshape(-1)          # device order: [y][x]
    # device rows are pitch floats long; host rows nx: with nx % 64 == 0 they coincide
    strips = (n + 255) // 256 if depth == 4 else (n + 239) // 240      # (k_step5, k_deep: 240 apart)
    wpc = 8 if depth < 6 else 4                   # (the waves per CU the library sizes the launch for: launch_step2)
    cap = 256 * wpc // 2                          # an item = a pair of segments = one workgroup of two waves (up / down)
    segs = max(cap // strips, 1)
    seg_rows = max(-(-ny // segs), 8)
    segs = -(-ny // seg_rows)
    items = 2 * strips * segs
    if deep2:
        return deep2_report(u, strips, segs, n, ny)
    # (boxes with walls: the first / last strip march shorter segments, their extra items follow: read what is there)
    items = min(items + 8 * segs, u.size // 8)
    rec = u[:8 * items].reshape(items, 8).astype(np.int64)
    t0 = rec[:, 0] | (rec[:, 1] << 32)
    t1 = rec[:, 2] | (rec[:, 3] << 32)
    ok = (rec[:, 6] == np.arange(items)) & (t1 > t0)
    print("grid %d x %d: wave records %d, valid %d, pairs per strip %d, rows per pair %d" % (n, ny, items, int(ok.sum()), segs, seg_rows))
    t0, t1, rec = t0[ok], t1[ok], rec[ok]
    base = t0.min()
    start, end = (t0 - base) / 100.0, (t1 - base) / 100.0            # microseconds
    xcc = rec[:, 4] & 15
    print("launch span %.1f us; wave start: median %.1f max %.1f us; wave end: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f us"
          % (end.max(), np.median(start), start.max(), end.min(), np.percentile(end, 10), np.median(end),
             np.percentile(end, 90), end.max()))
    print("mean residency of a wave slot: %.1f %% of the launch" % (100 * (end - start).mean() / end.max()))
    for x in range(8):
        m = xcc == x
        if m.any():
            print("XCD %d: %4d waves, end median %.1f  p90 %.1f  max %.1f us" % (x, m.sum(), np.median(end[m]), np.percentile(end[m], 90), end[m].max()))
    hw = rec[:, 5]
    simd, wave_slot, cu = (hw >> 4) & 3, hw & 15, (hw >> 8) & 15          # HW_ID: wave_id[3:0] simd_id[5:4] pipe[7:6] cu_id[11:8] sh[12] se[15:13]
    for sd in range(4):
        m = simd == sd
        if m.any():
            print("SIMD %d: %4d waves, end median %.1f us; share of upward waves: %.2f" % (sd, m.sum(), np.median(end[m]), (rec[m, 6] % 2).mean()))
    for ws in sorted(set(wave_slot.tolist())):
        m = wave_slot == ws
        print("wave slot %d: %4d waves, end median %.1f us" % (ws, m.sum(), np.median(end[m])))
    it_id = rec[:, 6] >> 1                                            # the pair; bit 0 = direction (0 down, 1 up)
    for d, name in ((0, "down"), (1, "up")):
        m = (rec[:, 6] & 1) == d
        if m.any():
            print("%-4s waves: start median %.1f us, end median %.1f us, duration median %.1f us" % (
                name, np.median(start[m]), np.median(end[m]), np.median((end - start)[m])))
    nseg_main = int(os.environ.get("LB_TIMELINE_NSEGS", segs))       # segments of the interior strips (= segs unless walls)
    sx = np.where(it_id < strips * nseg_main, it_id % strips, np.where((it_id - strips * nseg_main) & 1, strips - 1, 0))
    sy = np.where(it_id < strips * nseg_main, it_id // strips, nseg_main + ((it_id - strips * nseg_main) >> 1))
    order = np.argsort(-end)[:24]
    print("slowest waves (end us, strip, segment, XCD, CU, SIMD, slot):",
          " ".join("(%.0f,%d,%d,%d,%d,%d,%d)" % (end[i], sx[i], sy[i], xcc[i], cu[i], simd[i], wave_slot[i]) for i in order))
    print("end by strip (max us):", " ".join("%.0f" % end[sx == i].max() for i in range(strips)))
    print("end by strip (median us):", " ".join("%.0f" % np.median(end[sx == i]) for i in range(strips)))
    print("end by segment (median us), first 16:", " ".join("%.0f" % np.median(end[sy == i]) for i in range(min(segs, 16))))


def deep2_report(u, strips, segs, n, ny):
    # (boxes with walls: the wall strips' edge items follow the interior's, in other numbers than `segs`: read what is there)
    items = min(4 * (strips * segs + 8 * segs), u.size // 8)
    rec = u[:8 * items].reshape(items, 8).astype(np.int64)
    t0 = rec[:, 0] | (rec[:, 1] << 32)
    t1 = rec[:, 2] | (rec[:, 3] << 32)
    ok = (rec[:, 6] == np.arange(items)) & (t1 > t0)
    print("k_deep2, grid %d x %d: wave records %d, valid %d, pairs per strip %d" % (n, ny, items, int(ok.sum()), segs))
    t0, t1, rec = t0[ok], t1[ok], rec[ok]
    base = t0.min()
    start, end = (t0 - base) / 100.0, (t1 - base) / 100.0
    print("launch span %.1f us; wave start: median %.1f p90 %.1f max %.1f us; wave end: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f us"
          % (end.max(), np.median(start), np.percentile(start, 90), start.max(), end.min(), np.percentile(end, 10), np.median(end),
             np.percentile(end, 90), end.max()))
    print("mean residency of a wave: %.1f %% of the launch" % (100 * (end - start).mean() / end.max()))
    role = rec[:, 6] & 3
    for r, name in enumerate(("front down", "front up", "back down", "back up")):
        m = role == r
        print("%-10s: %4d waves, start median %.1f, end median %.1f p90 %.1f max %.1f us, duration median %.1f us" % (
            name, m.sum(), np.median(start[m]), np.median(end[m]), np.percentile(end[m], 90), end[m].max(), np.median((end - start)[m])))
    hw = rec[:, 5]
    simd, cu, se, xcc = (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 13) & 7, rec[:, 4] & 15
    key = ((xcc * 8 + se) * 16 + cu) * 2 + ((hw >> 12) & 1)
    per_cu = {}
    for k, e in zip(key.tolist(), end.tolist()):
        per_cu.setdefault(k, []).append(e)
    counts = np.array([len(v) for v in per_cu.values()])
    print("CUs holding waves: %d; waves per CU: %s" % (len(per_cu), dict(zip(*np.unique(counts, return_counts=True)))))
    for c in sorted(set(counts.tolist())):
        ends = np.array([max(v) for v in per_cu.values() if len(v) == c])
        print("  CUs with %d waves: last wave ends median %.1f max %.1f us" % (c, np.median(ends), ends.max()))
    # the two workgroups of a CU (a workgroup = the four waves of an item; its end = its last wave's): which ends first, and how far apart
    wg = rec[:, 6] >> 2
    per_cu_wg = {}
    for k, g, e in zip(key.tolist(), wg.tolist(), end.tolist()):
        d = per_cu_wg.setdefault(k, {})
        d[g] = max(d.get(g, 0.0), e)
    two = np.array([sorted(d.values()) for d in per_cu_wg.values() if len(d) == 2])
    if len(two):
        gap = two[:, 1] - two[:, 0]
        print("CUs with two workgroups: %d; first to end: median %.1f us, second: median %.1f us; gap median %.1f p10 %.1f p90 %.1f us = "
              "%.1f %% of the launch (median)" % (len(two), np.median(two[:, 0]), np.median(two[:, 1]), np.median(gap),
                                                 np.percentile(gap, 10), np.percentile(gap, 90), 100 * np.median(gap) / end.max()))
        # does the workgroup launched first (the lower item on the CU) end first?  (a stable sign is what a static bias would need)
        first_low = np.array([min(d, key=d.get) == min(d) for d in per_cu_wg.values() if len(d) == 2])
        print("  the workgroup with the lower item number ends first on %d of %d such CUs" % (int(first_low.sum()), len(first_low)))
    # what shares a SIMD: a front wave and a back wave (the role rotation of k_deep2), or two of a kind
    per_simd = {}
    for k, sd, r in zip(key.tolist(), simd.tolist(), role.tolist()):
        per_simd.setdefault((k, sd), []).append(r >> 1)
    pairs = [sorted(v) for v in per_simd.values() if len(v) == 2]
    print("SIMDs holding two waves: %d; a front and a back wave on %d, two front waves on %d, two back waves on %d" % (
        len(pairs), pairs.count([0, 1]), pairs.count([0, 0]), pairs.count([1, 1])))
    # how the roles were taken (kernels_deep2.h: deep2_take_role): record [7] bit 29 = by SIMD, bit 30 = the workgroup's flip
    by_simd, flip = (rec[:, 7] >> 29) & 1, (rec[:, 7] >> 30) & 1
    per_wg = {}
    for g, sd, r, b in zip(wg.tolist(), simd.tolist(), role.tolist(), by_simd.tolist()):
        per_wg.setdefault(g, []).append((sd, r, b))
    whole = [v for v in per_wg.values() if len(v) == 4]
    perm = [v for v in whole if sorted(x[0] for x in v) == [0, 1, 2, 3]]
    follows = [v for v in perm if len({(x[1] - x[0]) & 3 for x in v}) == 1 and ((v[0][1] - v[0][0]) & 1) == 0]
    print("workgroups: %d; roles by SIMD in %d; their four waves on four different SIMDs in %d; role = SIMD (+ 2 under flip) in %d" % (
        len(whole), sum(1 for v in whole if v[0][2]), len(perm), len(follows)))
    cu_flip = {}
    for k, g, fl in zip(key.tolist(), wg.tolist(), flip.tolist()):
        cu_flip.setdefault(k, {})[g] = fl
    twof = [sorted(d.values()) for d in cu_flip.values() if len(d) == 2]
    print("CUs with two workgroups: flip 0 and 1 on %d, both 0 on %d, both 1 on %d" % (twof.count([0, 1]), twof.count([0, 0]), twof.count([1, 1])))
    hist, edges = np.histogram(end, bins=12)
    print("wave ends, histogram:", " ".join("%.0f-%.0f:%d" % (edges[i], edges[i + 1], hist[i]) for i in range(len(hist))))
    hist, edges = np.histogram(start, bins=8)
    print("wave starts, histogram:", " ".join("%.0f-%.0f:%d" % (edges[i], edges[i + 1], hist[i]) for i in range(len(hist))))


if __name__ == "__main__":
    main()
