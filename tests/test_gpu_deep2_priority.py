"""k_deep2<7> under its static issue priority (csrc/kernels_deep2.h: deep2_set_prio) against the single-step kernel, bit for bit.

Results cannot depend on a wave's issue priority, but the kernel's hand-written barrier protocol -- two barriers per trip, the
hand-over slot, the links the two directions publish for each other -- now runs under another timing: with the back waves raised
(the mode that ships) the two workgroups of a CU advance in step instead of one after the other, every wave meets another pace in
the wave it shares a SIMD with, and anything the protocol left to luck would show as wrong bits.  Every case runs 7 + 14 steps, three launches of the seven-step kernel, on handles that store rho, u, v with the last
launch of a run (eager_macro), and compares f, rho, u, v of K_DEEP2 with K_STEP's after each run.

Shapes.  The first table is the one the change was specified with: 496 (497 in a walled box) columns = two strips of 240 and a
16-column remainder strip that holds the periodic seam, 224 and 112 rows.  The marching kernels take boxes of at least 512 columns
and 128 rows (csrc/plan.cpp: step4_applicable); on a smaller box a forced word runs the single-step kernel, so those cases compare
k_step with itself and only pin that the word stays harmless there.  The second table is the same geometry at the smallest sizes
k_deep2<7> does run at -- 736 = 3 x 240 + 16 (737 walled) columns, 224 and 128 rows: a 16-column remainder strip with the seam,
segment pairs of eight rows, i.e. marches of four rows behind seven trips of fill -- and there the kernel's name is asserted."""
import numpy as np
import pytest

from kernel_variants import assert_forced_kernel, same_bits
from LB_D2Q9.variants import K_DEEP2, K_STEP
from test_gpu_parity import _random_state

pytestmark = pytest.mark.gpu

FIELDS = ("f", "rho", "u", "v")
KW = {"periodic": {}, "pipe": dict(inlet_rho=1.004, outlet_rho=1.0), "cavity": dict(lid_u=0.06, rho0=1.0)}

# (family, nx, ny, mask): the shapes as specified / the smallest k_deep2<7> runs at
SPECIFIED = [("periodic", 496, 224, None), ("periodic", 496, 224, "random"), ("periodic", 496, 112, None), ("periodic", 496, 112, "random"),
             ("pipe", 497, 224, "disc"), ("cavity", 497, 224, None)]
MARCHED = [("periodic", 736, 224, None), ("periodic", 736, 224, "random"), ("periodic", 736, 128, None), ("periodic", 736, 128, "random"),
           ("pipe", 737, 224, "disc"), ("cavity", 737, 224, None)]


def _mask(kind, rng, nx, ny):
    if kind is None:
        return None
    if kind == "random":
        return rng.random((nx, ny)) < 0.01
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    # a disc across the boundary of the second strip and the remainder strip, clear of the walls
    return (x - (nx - 20)) ** 2 + (y - ny // 2) ** 2 <= (ny // 8) ** 2


def _engine(bc, nx, ny, mask, f0, variant):
    from LB_D2Q9.simulation import Simulation
    s = Simulation(nx, ny, 1.6, bc=bc, obstacle_mask=mask, eager_macro=True, **KW[bc])
    s.set_variant(variant)
    s.set_f(f0)
    return s


def _run_case(bc, nx, ny, kind, marched):
    rng = np.random.default_rng(nx * 1000 + ny + (7 if kind else 0))
    mask = _mask(kind, rng, nx, ny)
    f0 = _random_state(rng, nx, ny)
    one, deep = _engine(bc, nx, ny, mask, f0, K_STEP), _engine(bc, nx, ny, mask, f0, K_DEEP2)
    try:
        if marched:
            assert_forced_kernel(deep, K_DEEP2)
            assert deep.plan_launches(7) == [7] and deep.plan_launches(14) == [7, 7], (deep.plan_launches(7), deep.plan_launches(14))
        for n in (7, 14):
            one.run(n)
            deep.run(n)
            same_bits(deep.get_fields(FIELDS), one.get_fields(FIELDS), (bc, nx, ny, kind, n), FIELDS)
    finally:
        one.close()
        deep.close()


@pytest.mark.parametrize("bc,nx,ny,kind", SPECIFIED)
def test_deep2_word_bitwise_on_the_specified_shapes(lbhip, bc, nx, ny, kind):
    """The table the change was specified with (below the marching kernels' smallest box: see the module's text)."""
    _run_case(bc, nx, ny, kind, marched=False)


@pytest.mark.parametrize("bc,nx,ny,kind", MARCHED)
def test_deep2_bitwise_with_remainder_strip_and_short_marches(lbhip, bc, nx, ny, kind):
    """The same geometry at the smallest sizes k_deep2<7> runs at; the kernel's name and the 7 + 7 + 7 plan are asserted."""
    _run_case(bc, nx, ny, kind, marched=True)
