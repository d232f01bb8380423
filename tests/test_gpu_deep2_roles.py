"""k_deep2<7> with its waves' roles taken from the SIMD each wave runs on (csrc/kernels_deep2.h: deep2_take_role, csrc/deep2_roles.h)
against the single-step kernel, bit for bit.

Which of the four bodies -- front-down, front-up, back-down, back-up -- a wave enters is now decided at run time, from four words
the waves of a workgroup publish in LDS behind one more barrier.  No arithmetic changes, so f, rho, u, v must stay K_STEP's to the
bit; what could go wrong is the protocol: two waves in one body (a race on the LDS windows), a wave that takes the down march with
the up march's windows, a workgroup that reaches the new barrier with fewer than four waves.  Every case runs 7, then 14 steps
(three launches of the seven-step kernel) on handles that store rho, u, v with the last launch of a run (eager_macro).

Shapes.  The first table holds the smallest boxes k_deep2<7> runs at: 736 = 3 x 240 + 16 columns (737 walled) -- a 16-column
remainder strip --, 128 and 224 rows: segment pairs of eight rows; the pipe and the cavity have the wall strips' edge items, and
workgroups past the last row that return before the new barrier.  All of these launch fewer than 256 workgroups: one per CU, one
value of the launch-order bit.  The second table is 768 x 1024 periodic: four strips (3 x 240 + 48), 512 wave slots / 4 strips = 128
segment pairs of eight rows each, i.e. 4 x 128 = 512 workgroups (csrc/plan.cpp: plan_march; the per-wave timeline of that launch
holds 2048 valid records: profiles/deep2_roles_ab.txt) -- two on every CU of a 256-CU device, both values of the launch-order bit,
and the two workgroups of a CU must take opposite halves of the SIMDs."""
import numpy as np
import pytest

from kernel_variants import assert_forced_kernel, same_bits
from LB_D2Q9.variants import K_DEEP2, K_STEP
from test_gpu_parity import _random_state

pytestmark = pytest.mark.gpu

FIELDS = ("f", "rho", "u", "v")
KW = {"periodic": {}, "pipe": dict(inlet_rho=1.004, outlet_rho=1.0), "cavity": dict(lid_u=0.06, rho0=1.0)}

# (family, nx, ny, mask)
SMALLEST = [("periodic", 736, 128, None), ("periodic", 736, 128, "random"), ("periodic", 736, 224, None), ("periodic", 736, 224, "random"),
            ("pipe", 737, 224, "disc"), ("cavity", 737, 224, None)]
TWO_PER_CU = [("periodic", 768, 1024, None), ("periodic", 768, 1024, "random")]


def _mask(kind, rng, nx, ny):
    if kind is None:
        return None
    if kind == "random":
        return rng.random((nx, ny)) < 0.01
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    # a disc across the boundary of the last whole strip and the remainder strip, clear of the walls
    return (x - (nx - 20)) ** 2 + (y - ny // 2) ** 2 <= (ny // 8) ** 2


def _engine(bc, nx, ny, mask, f0, variant):
    from LB_D2Q9.simulation import Simulation
    s = Simulation(nx, ny, 1.6, bc=bc, obstacle_mask=mask, eager_macro=True, **KW[bc])
    s.set_variant(variant)
    s.set_f(f0)
    return s


def _run_case(bc, nx, ny, kind):
    rng = np.random.default_rng(nx * 1000 + ny + (11 if kind else 0))
    mask = _mask(kind, rng, nx, ny)
    f0 = _random_state(rng, nx, ny)
    one, deep = _engine(bc, nx, ny, mask, f0, K_STEP), _engine(bc, nx, ny, mask, f0, K_DEEP2)
    try:
        assert_forced_kernel(deep, K_DEEP2)
        assert deep.plan_launches(7) == [7] and deep.plan_launches(14) == [7, 7], (deep.plan_launches(7), deep.plan_launches(14))
        for n in (7, 14):
            one.run(n)
            deep.run(n)
            same_bits(deep.get_fields(FIELDS), one.get_fields(FIELDS), (bc, nx, ny, kind, n), FIELDS)
    finally:
        one.close()
        deep.close()


@pytest.mark.parametrize("bc,nx,ny,kind", SMALLEST)
def test_deep2_roles_bitwise_on_the_smallest_boxes(lbhip, bc, nx, ny, kind):
    """Remainder strip, wall strips' edge items, workgroups that return before the roles' barrier; one workgroup per CU."""
    _run_case(bc, nx, ny, kind)


@pytest.mark.parametrize("bc,nx,ny,kind", TWO_PER_CU)
def test_deep2_roles_bitwise_with_two_workgroups_per_cu(lbhip, bc, nx, ny, kind):
    """512 workgroups (more than 256: both values of the launch-order bit), two on every CU."""
    _run_case(bc, nx, ny, kind)
