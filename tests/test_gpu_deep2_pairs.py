"""k_deep2<7> with its steady trips run in pairs (csrc/kernels_deep2.h: deep2_front, deep2_back, deep2_pairs_front / _back) against
the single-step kernel, bit for bit.

In a periodic box without an obstacle mask both roles run their steady trips two to a loop body: an unconditional paired loop while
two more trips lie inside the wave's own positions, then the guarded single-trip loop for the rest.  No arithmetic changes; what can
go wrong is the trip counts -- a pair that runs past a wave's last position, a rest that runs a position with the wrong parity of
the LDS ring, the four waves of a workgroup out of step at the two barriers of a trip because their loops differ.  The existing
k_deep2 tests at small shapes mostly carry an obstacle mask, which is another instantiation; these cases carry none:

  512 x 128            segment pairs of 8 rows, halves 4 / 4: a front wave runs 7 steady trips (three pairs + one), a back wave 4 (two pairs)
  964 x 129, 130, 131  the last pair holds 1, 2, 3 rows, halves 0 / 1, 1 / 1, 1 / 2: its back waves get 0 or 1 steady trips -- no pair
                       at all --, and the two directions of a workgroup differ by one trip
  964 x 864            segments of NINE rows, halves 4 / 5 in every workgroup: the up waves run one steady trip more than the down
                       waves, i.e. a front-up wave four pairs where front-down runs three pairs + one

and one pipe and one cavity at 737 x 128 and one periodic box with a mask at 736 x 128: the instantiations that stay unpaired (paired
they spill) run the same source through the other arm of the same `if constexpr`.
The segment rows are the planner's on 256 CUs (`plan_props --classify`, tests/plan_props.cpp); the first test holds the table to them
on a host.  Every case: run(7), run(14), run(1), fields compared after each, rho, u, v rebuilt on demand and stored by the last launch
of a run (eager_macro: the back wave's MACRO instantiation).

HALVES: a wave of n rows runs n + 3 steady trips as a front wave (n + 6 positions, three of them while the pipeline fills) and n as a
back wave (n + 3, three filling): 4 -> 7 and 4, 5 -> 8 and 5, 0 / 1 / 2 -> 3 / 4 / 5 and 0 / 1 / 2."""
import subprocess

import numpy as np
import pytest

from kernel_variants import assert_forced_kernel, same_bits
from march_shapes import class_fields, classify_args, row_id
from test_plan_cpu import plan_props  # noqa: F401  (the fixture: tests/plan_props.cpp compiled on the host)
from LB_D2Q9.variants import K_DEEP2, K_STEP

FIELDS = ("f", "rho", "u", "v")
KW = {"periodic": {}, "pipe": dict(inlet_rho=1.004, outlet_rho=1.0), "cavity": dict(lid_u=0.06, rho0=1.0)}
RUNS = (7, 14, 1)

# (family, nx, ny, word, class) as tests/march_shapes.py, then the mask
CASES = [
    (("periodic", 512, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=48+0 wgs=48+0 strips=3 segs=16 row_begin=0"), None),
    (("periodic", 964, 129, K_DEEP2, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"), None),
    (("periodic", 964, 130, K_DEEP2, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"), None),
    (("periodic", 964, 131, K_DEEP2, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"), None),
    (("periodic", 964, 864, K_DEEP2, "seg_rows=9 last=9 edge_seg_rows=0 edge_last=0 extra=0 items=32+64k wgs=32+64k strips=5 segs=96 row_begin=0"), None),
    (("pipe", 737, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"), None),
    (("cavity", 737, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"), None),
    (("periodic", 736, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"), "random"),
]
# the halves (rows of the down / the up waves) of an interior and of the last segment pair, as the kernel cuts them: ym = ya + (yb - ya) / 2
HALVES = {(512, 128): ((4, 4), (4, 4)), (964, 129): ((4, 4), (0, 1)), (964, 130): ((4, 4), (1, 1)), (964, 131): ((4, 4), (1, 2)),
          (964, 864): ((4, 5), (4, 5))}


def _case_id(case):
    row, kind = case
    return row_id(row) + ("-mask" if kind else "")


def test_the_shapes_have_the_segments_the_trip_counts_are_read_from(plan_props):  # noqa: F811
    for row, _ in CASES:
        run = subprocess.run([plan_props, "--classify"] + classify_args(row), capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stdout.strip() == row[4], (row_id(row), run.stdout.strip(), row[4])
        c = class_fields(row[4])
        assert c["edge_seg_rows"] == 0 and c["extra"] == 0, row_id(row)          # (one kind of item: every workgroup a segment pair)
        if (row[1], row[2]) in HALVES:
            assert row[0] == "periodic"
            got = tuple((n // 2, n - n // 2) for n in (c["seg_rows"], c["last"]))
            assert got == HALVES[(row[1], row[2])], (row_id(row), got)


def _state(row, kind):
    bc, nx, ny = row[:3]
    rng = np.random.default_rng(nx * 1000 + ny + (11 if kind else 0))
    mask = (rng.random((nx, ny)) < 0.01) if kind else None
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, np.float32)
    f0 = w[None, None, :] * (1 + np.float32(0.02) * rng.standard_normal((nx, ny, 9), dtype=np.float32))
    return f0, mask


def _fields_after_each_run(row, state, eager, word):
    from LB_D2Q9.simulation import Simulation
    bc, nx, ny = row[:3]
    f0, mask = state
    s = Simulation(nx, ny, 1.6, bc=bc, obstacle_mask=mask, eager_macro=eager, **KW[bc])
    try:
        s.set_variant(word)
        s.set_f(f0)
        if word != K_STEP:
            assert_forced_kernel(s, word)
            assert s.plan_launches(7) == [7] and s.plan_launches(14) == [7, 7] and s.plan_launches(1) == [1], s.plan_launches(14)
        out = []
        for n in RUNS:
            s.run(n)
            out.append(s.get_fields(FIELDS))
        return out
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_deep2_paired_trips_bitwise(lbhip, case, eager):
    row, kind = case
    state = _state(row, kind)
    want = _fields_after_each_run(row, state, eager, K_STEP)
    got = _fields_after_each_run(row, state, eager, K_DEEP2)
    for n, g, w in zip(RUNS, got, want):
        same_bits(g, w, (_case_id(case), "eager" if eager else "lazy", "after run(%d)" % n), FIELDS)
