"""The marching kernels at shapes chosen for the geometry of their launch (tests/march_shapes.py: the wall split at its onset and
with one-row tails, shorter wall segments, tails of 1 ... 3 rows at every depth, item counts below, at and above one XCD-transposed
block), bit for bit against k_step.  This is the tie between the kernels' five item decodes and the one restatement that
tests/plan_props.cpp sweeps on a host.

Per row: random populations, a 1 % obstacle mask, and solid cells in the columns beside both walls (and in one interior column) at
the first and the last row of every wall segment and every interior segment -- walls and corners stay fluid in the walled families --;
the word is forced and held to the kernel it names; run(2 depth) is held, by the handle's own plan (lb_plan_launches), to two
launches of that depth -- a run of 2 depth + 1 steps would be split otherwise from five steps on (11 = 3 + 4 + 4, 13 = 4 + 4 + 5,
15 = 4 + 4 + 7: the planner's cheapest split), and k_step5 and k_deep<6> never launched at their own shapes --; run(1) follows, a
single step; rho, u, v rebuilt on demand, and stored by the last launch (eager macro); f, rho, u, v equal a k_step twin's in every bit.  Once per family the
twin is held to the oracle within the parity contract (contract_tol, test_gpu_parity.py) at the family's smallest shape.

Planted geometry defects (a library linked with a scratch plan.cpp, this file alone on the MI355X; of 136 + 4 cases):
  segs = rows / seg_rows (rounded down)      48 red, 92 green.  Red: the 24 rows without a wall split whose last segment is short, lazy
                                             and eager -- the tails of 1, 2 and 3 rows at every depth and 964 x 211 by the deep kernels;
                                             they are the 24 rows whose class the defect changes on a host.  Green: the walled rows,
                                             where the split's own lines count the segments again, rounded up, and 512 x 128, 724 x 128
  the `if (extra_items < 0)` line removed    none red: the line is dead code (tests/test_plan_cpu.py), every plan is the same
  `if (se < si) continue` removed            none red: on 256 CUs no shape of the table has a candidate of se = 0, and a split of
                                             se < si never passes `segs_e > segs_i` -- every plan of the table is the same; the host
                                             sweep dies of the division by zero at other CU counts and widths

Time: the file takes 30 s on an MI355X (the largest case is 964 x 4185).
"""
import numpy as np
import pytest

from kernel_variants import assert_forced_kernel, same_bits
from march_shapes import SHAPES, class_fields, row_id
from test_gpu_parity import assert_fields_close, contract_tol
from LB_D2Q9.variants import K_STEP, depth_of

pytestmark = pytest.mark.gpu

OMEGA = 1.55
KW = dict(pipe=dict(inlet_rho=1.003, outlet_rho=0.999), periodic={}, cavity=dict(lid_u=0.05), velocity_inlet=dict(inlet_u=0.03, outlet_u=0.028))

_state = {}         # _state_key -> (f0, mask, u0, v0) of the shape in hand: one at a time, the big ones take a second to draw
_twins = {}         # (_state_key, depth, eager) -> k_step's fields after run(2 depth), run(1); the last few only


def _segment_rows(c, ny):
    """First and last row of every interior and every wall segment of the row's launch."""
    lo, hi = c["row_begin"], ny - c["row_begin"]
    rows = set()
    for step in (c["seg_rows"], c["edge_seg_rows"]):
        if step > 0:
            starts = np.arange(lo, hi, step)
            rows.update(starts.tolist())
            rows.update(np.minimum(starts + step, hi) - 1)
    return np.array(sorted(rows))


def _state_key(bc, nx, ny, c):
    return (bc, nx, ny, c["seg_rows"], c["edge_seg_rows"], c["row_begin"])


def _shape_state(bc, nx, ny, c):
    key = _state_key(bc, nx, ny, c)
    if key not in _state:
        _state.clear()
        rng = np.random.default_rng(nx * 10007 + ny)
        w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, np.float32)
        f0 = w[None, None, :] * (1 + np.float32(0.02) * rng.standard_normal((nx, ny, 9), dtype=np.float32))
        mask = rng.random((nx, ny), dtype=np.float32) < 0.01
        rows = _segment_rows(c, ny)
        for x in (1, nx - 2, nx // 2 + 3):
            mask[x, rows] = True
        if bc != "periodic":
            mask[0, :] = mask[-1, :] = False
            mask[:, 0] = mask[:, -1] = False
        u0 = v0 = None
        if bc == "velocity_inlet":          # (its inlet and outlet columns read the stored u, v)
            u0 = np.float32(0.01) * rng.standard_normal((nx, ny), dtype=np.float32)
            v0 = np.float32(0.01) * rng.standard_normal((nx, ny), dtype=np.float32)
        _state[key] = (f0, mask, u0, v0)
    return _state[key]


def _run(bc, nx, ny, word, depth, eager, state, max_depth):
    from LB_D2Q9.simulation import Simulation
    f0, mask, u0, v0 = state
    s = Simulation(nx, ny, OMEGA, bc=bc, obstacle_mask=mask, eager_macro=eager, **KW[bc])
    s.set_variant(word)
    if word != K_STEP:
        assert_forced_kernel(s, word, max_depth=max_depth)
    if u0 is not None:
        s.set_fields(np.ones((nx, ny), np.float32), u0, v0)
    s.set_f(f0)
    if word != K_STEP:      # the two launches the row is in the table for, and nothing else
        assert s.plan_launches(2 * depth) == [depth, depth] and s.plan_launches(1) == [1], (word, s.plan_launches(2 * depth))
    s.run(2 * depth)
    s.run(1)
    out = s.get_fields(("f", "rho", "u", "v"))
    s.close()
    return out


def _twin(state_key, depth, eager, state):
    key = (state_key, depth, eager)
    if key not in _twins:
        while len(_twins) >= 2:
            _twins.pop(next(iter(_twins)))
        bc, nx, ny = state_key[:3]
        _twins[key] = _run(bc, nx, ny, K_STEP, depth, eager, state, 7)
    return _twins[key]


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("row", SHAPES, ids=row_id)
def test_marching_kernels_at_the_shapes_of_the_geometry_table(lbhip, row, eager):
    bc, nx, ny, word, cls = row
    c = class_fields(cls)
    depth = depth_of(word)
    state = _shape_state(bc, nx, ny, c)
    got = _run(bc, nx, ny, word, depth, eager, state, 5 if bc == "velocity_inlet" else 7)
    same_bits(got, _twin(_state_key(bc, nx, ny, c), depth, eager, state), row_id(row))


SMALLEST = {}
for _row in SHAPES:
    if _row[0] not in SMALLEST or _row[1] * _row[2] < SMALLEST[_row[0]][1] * SMALLEST[_row[0]][2]:
        SMALLEST[_row[0]] = _row


@pytest.mark.parametrize("bc", sorted(SMALLEST))
def test_the_twin_follows_the_oracle(lbhip, oracle, bc):
    """k_step itself, at the family's smallest shape of the table, against the CPU oracle within the parity contract."""
    _, nx, ny, word, cls = SMALLEST[bc]
    depth = depth_of(word)
    steps = 2 * depth + 1
    state = _shape_state(bc, nx, ny, class_fields(cls))
    f0, mask, u0, v0 = state
    code = dict(pipe=oracle.BC_PIPE, periodic=oracle.BC_PERIODIC, cavity=oracle.BC_CAVITY, velocity_inlet=oracle.BC_VELOCITY_INLET)[bc]
    kw = KW[bc]
    if bc == "velocity_inlet":
        o = oracle.O2Sim(nx, ny, OMEGA, code, u_w=kw["inlet_u"], u_e=kw["outlet_u"], mask=mask)
        o.set_macro(np.ones((nx, ny)), u0, v0)
    else:
        o = oracle.O2Sim(nx, ny, OMEGA, code, kw.get("inlet_rho", 1.), kw.get("outlet_rho", 1.), kw.get("lid_u", 0.), 1., mask=mask)
    o.set_f(f0)
    o.run(steps)
    assert_fields_close(_twin(_state_key(bc, nx, ny, class_fields(cls)), depth, False, state), o.get_fields(), contract_tol(steps))
