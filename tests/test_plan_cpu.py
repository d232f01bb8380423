"""The launch planner (2d-lb_amd/csrc/plan.cpp) on a host: tests/plan_props.cpp -- its own main, plan.h, linked with plan.cpp only --
is compiled with the host compiler and run, plain on the whole sweep and under the address and undefined-behaviour sanitizers on a
thinner one (`--thin`: every third height, a third of the boxes and words; a stand-alone program, nothing is preloaded).  The program
restates the kernels' item decode once and sweeps CU counts {256, 304, 64, 8} x the four boundary families x depths 2 ... 7 x
lb_autotune's waves per CU {0, 4, 6, 8} x widths 512 ... 9000 x 1 ... 8192 rows x the reserve {0, launch_interior's}:

  P1  every output row of every strip exactly once -- balanced launches, and a slab's bands and interiors as slab.cpp forms them
      (launch_bands, launch_interior, slab_step_launch, both halves of the halo cycle, one launch per band and split); segs, seg_rows,
      items >= 1; no empty item below strips x segs; a width reaches plan_march through march_strips alone
  P2  items <= max(capacity, strips); a wall split has >= 8 rows per wave and, where its segments are shorter than the interior's,
      more of them (where the planner's two slot counts round to the same rows -- 964 x 3856 by k_step4: 16 and 16 -- the split says
      what no split says: same segments, no extra item; the issue's "segs_e > segs_i" read on what the kernels are handed)
  P3  band_extra: even, >= 0, 0 below four steps; B > 0 leaves the second interior >= 16 rows and the bands apart
  P4  plan_launches: sums to n, only depths that whole_grid_depths allows and the handle can run, none >= 6 in the velocity-inlet
      family, steps_per_launch = the deepest of a long run; scalar / porous / multifluid / rocket handles: 4 a + r or single steps
  P5  next_advance: the split it leads to costs what a brute-force minimum costs (exactly, on costs that binary32 adds exactly), the
      tie rule (the cheapest split whose shallowest launch is deepest, shallow launches first), the deepest depth beyond 64 steps
  P6  ranks of one run (same box, family, min_h, number of ranks, word, cycle, flavour, transport) that differ in mask, own height,
      place, bytes and CU count agree on cycle_depth, slab_step_depths, deep2_chosen
  P7  tune_entry_runs_here only where launch_march has the kernel; what cycle_depth returns can run; planes that do not fit: no
      marching depth anywhere; an evenly shared planar run decides on its slabs' own planes
  P8  hot_kernel ends inside buffers of 1, 8, 64 and 512 bytes and names what steps_per_launch, use_tile_kernel, deep2_chosen imply

What the sweep found in the planner as it was: P6.  The plane stride of an LB_FLAG_PLANAR slab grows with the slab's own height, and
marching_planes_fit read it: of two slabs of a planar 12288^2 box, 11264 and 1024 rows, the tall one dropped the halo cycle (depth 0)
that the short one kept (5) -- with the slab's own plane as before, 15 685 of 2.11 M cases of this sweep.  Fixed in plan.cpp: the
slabs of a run decide on the tallest slab that nranks slabs of at least min_h rows can hold, ny - (nranks - 1) min_h rows, which every
rank knows and which is the slab's own height where the rows are shared out evenly (P7 holds it to that: deciding on ny - min_h
rows whatever the number of ranks turns 34 560 cases red, evenly shared planar runs that lose their cycle for nothing).  An uneven
planar run whose tallest possible slab does not fit takes single steps although its real slabs might fit: not measured, boxes of
more than ~11000^2 cells in the planar layout only.  Everything else held.

Planted defects (one line of a scratch copy of plan.cpp each; the whole sweep; bad cases per property, all others 0):
  segs = rows / seg_rows (rounded down)       P1_coverage 3 438 531 of 5 364 480, P1_coverage_slab_launches 665 706 of 4 586 749 (the
                                              interiors): the last rows of every strip are never marched
  the `if (extra_items < 0)` line removed     none, and none can: a split is taken only with segs_e > segs_i, hence rows_e <= rows_i and
                                              ceil(rows / rows_e) >= ceil(rows / rows_i) = segs -- the line is dead code
  `if (se < si) continue` removed             the program dies in plan_march of a division by zero (se = 0 where the strips are many for the
                                              slots: strips^2 - strips >= 2 x capacity, few CUs or very wide boxes): red by exit status, and the sanitizer build names the line.
                                              With candidates of se >= 1 only: none -- a split of se < si never passes the later
                                              `segs_e > segs_i`
  `room` without its `- 8`                    none, and none can: the scan stops at band > inner first, and band <= inner alone gives
                                              H - 4D - 2b >= 2D + b + 16 (one launch per band) or >= 4D + b + 4 (split), >= 16 from D = 4
  cycle_depth reading s->H for h              P6_rank_agreement 308 209 of 2 109 240, P7_consistency 308 209 of 2 283 240
  deep_side reading has_mask on slabs         P6_rank_agreement 192 (periodic slabs between 2200^2 and 2400^2 cells, the planted threshold
  (2200 with a mask, 2400 without)            and the real one)
  next_advance without its tie rule           P5_tie_rule 684 of 12 160; P5_next_advance none (the split stays a cheapest one)
The three geometry defects on the MI355X: the docstring of tests/test_gpu_march_geometry.py.

Time: this file takes 31 s on a host (two compilations, 7 s of the whole sweep, 8 s of the thin one under the sanitizers).
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from march_shapes import SHAPES, class_fields, classify_args, row_id

CSRC = os.path.join(ROOT, "2d-lb_amd", "csrc")
PROPERTIES = ("xcd_item_permutes", "P1_coverage", "P1_width_only_through_strips", "P1_coverage_slab_launches", "P2_one_round", "P3_band_extra",
              "P4_plan_launches", "P5_next_advance", "P5_tie_rule", "P6_rank_agreement", "P7_consistency", "P8_hot_kernel")


def _compile(out, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + extra +
                          [os.path.join(ROOT, "tests", "plan_props.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def plan_props(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("plan_props") / "plan_props"), ["-O2"])


def _assert_all_hold(run):
    print(run.stdout)
    print(run.stderr[-3000:])
    found = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+) cases=(\d+) bad=(\d+)$", run.stdout, re.M)}
    for name in PROPERTIES:
        assert name in found, (name, "not reported")
        cases, bad = found[name]
        assert cases > 0 and bad == 0, (name, cases, bad, run.stdout[-3000:])
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])


def test_the_planner_keeps_its_invariants(plan_props):
    _assert_all_hold(subprocess.run([plan_props], capture_output=True, text=True, timeout=600))


def test_the_planner_keeps_its_invariants_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined (any report ends it: -fno-sanitize-recover), on the thin sweep: the
    planner reads and writes inside its arrays (next_advance's tables, hot_kernel's buffer, plan_launches' depths) and its integer
    arithmetic neither overflows nor divides by zero at any swept input."""
    exe = _compile(str(tmp_path / "plan_props_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = subprocess.run([exe, "--thin"], capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    _assert_all_hold(run)


def test_every_shape_of_the_gpu_table_is_in_the_class_it_claims(plan_props):
    for row in SHAPES:
        run = subprocess.run([plan_props, "--classify"] + classify_args(row), capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stdout.strip() == row[4], (row_id(row), run.stdout.strip(), row[4])


def test_the_gpu_table_holds_the_classes_it_is_there_for():
    cls = [(row, class_fields(row[4])) for row in SHAPES]
    from LB_D2Q9.variants import K_DEEP2, K_DEEP6, K_DEEP7, K_STEP2, K_STEP3, K_STEP4, K_STEP5
    walled = {K_STEP4: ("pipe", "cavity", "velocity_inlet"), K_STEP5: ("pipe", "cavity", "velocity_inlet"),
              K_DEEP6: ("pipe", "cavity"), K_DEEP7: ("pipe", "cavity"), K_DEEP2: ("pipe", "cavity")}
    for word, families in walled.items():
        for bc in families:
            mine = [c for r, c in cls if r[0] == bc and r[3] == word]
            assert any(c["edge_seg_rows"] > 0 for c in mine), (bc, word, "no wall split")
            assert any(c["edge_seg_rows"] > 0 and c["last"] == 1 and c["edge_last"] == 1 for c in mine), (bc, word, "no one-row tails")
        for bc in ("pipe", "velocity_inlet")[:2 if word in (K_STEP4, K_STEP5) else 1]:
            mine = [c for r, c in cls if r[0] == bc and r[3] == word]
            assert any(c["extra"] > 0 and c["last"] == 1 and c["edge_last"] == 1 for c in mine), (bc, word, "no shorter wall segments")
    for word in (K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_DEEP6, K_DEEP7, K_DEEP2):
        tails = {c["last"] for r, c in cls if r[0] == "periodic" and r[3] == word}
        assert {1, 2, 3} <= tails, (word, tails)
    for word in (K_DEEP6, K_DEEP7, K_DEEP2):
        counts = {c["wgs"] for r, c in cls if r[3] == word}
        assert "48+0" in counts and "0+64" in counts and any(c.endswith("+64") and c != "0+64" for c in counts) and \
            any(c.endswith("+64k") for c in counts), (word, counts)
