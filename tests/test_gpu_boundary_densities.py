"""Every boundary rule with outlet_rho, rho0 and the fluid's density off 1, in every kernel.

Every other GPU test passes outlet_rho = 1.0 and rho0 = 1.0 (or leaves the defaults) and starts from populations w_k (1 +- 2 %).
Two things cannot be seen there.  A rule that reads the wrong one of its densities -- the marching kernels' out-of-line rule gets
them as two anonymous floats (kernels_fused.h collide_row: `cav ? a.lid_u : a.rho_in, cav ? a.rho0 : a.rho_out`), the corner
closures and the Cython path's moment overrides name them once each, StepArgs and PhaseArgs are filled in two places (launch.cpp,
lb_hip.cpp) -- computes the same when both are 1.  And `x / rout`, `(2/3) rout uu`, `(1/6) uu rout` each lose a rounding step at
rout == 1.

Parameter sets (PIPE, CAVITY, FORK below): densities within 0.9 ... 1.1, so that w_k rho stays in the binade w_k occupies at
density 1 (4/9 rho in [0.25, 0.5), 1/9 rho in [0.0625, 0.125), 1/36 rho in [2^-6, 2^-5)): one rounding has the size it has in every
other test, and the project's parity contract applies unchanged -- TOL1, TOLN, contract_tol(n) of test_gpu_parity.py.  The state
is rho_fluid x _random_state(...), rho_fluid = the outlet's density / rho0.  All cells are compared.

CPU facts this file relies on (established with the oracle, which tests/test_oracle_golden.py pins off 1 bit for bit against
the executed reference: o2_offone_37x19, o2_d2q9i_offone_37x19):
  * stability: 2 % noise, omega 1.6, 5 % masks, 5 x 7 ... 130 x 130, up to 19 steps, pipe at (0.9337, 0.93) and cavity at
    (0.06, 1.07): all finite, max |u| 0.06, rho within 0.90 ... 1.11;
  * sensitivity: the same run with the parameter put back to 1 moves f by 3e-2 ... 5e-2 after ONE step, on exactly the ny cells
    of the outlet column (pipe) / the 4 corner cells (cavity: rho0 only ever touches the corners): a kernel that ignores the
    parameter is four orders of magnitude outside the contract.  NOT_VACUOUS below is a fifth of that;
  * the incompressible fork: a fluid density of 0.93 or 1.07 drives it to |u| ~ 0.4 by step 5 and NaN by step 10, so it runs
    at (1.0002, 0.9998), fluid at 1, noise 0.1 %, omega 1.0, where it behaves as in test_gpu_d2q9i.py for 8 steps (max |u| 0.0075,
    rho 0.968 ... 1.028; NaN by step 19); its sensitivity to outlet_rho is 1.8e-4 on f after 1 step and 2.3e-3 after 8 -- 18 and
    230 times the bound it is held to, so the oracle comparison is what bites there;
  * the Cython path: omega 1.3 (at 1.6 its plain bounce-back walls drive small boxes to NaN within 50 steps, oracle and product
    alike); tests/test_cpu_backend.py holds the CPU backend to the same oracle bit for bit at these densities.

The analytic property (assert_imposed_density, tests/test_oracle_golden.py): the pressure rules close a column's three unknown
links so that sum_k f = the imposed density, a corner's two free links get half of what the density lacks -- asserted in float64
on the DEVICE's populations after one move_bcs call, within 4 x 2^-24 rho.  The Cython path's inlet / outlet rule takes its
velocity from the stored u; with the u its own update_hydro derives from the same populations the same property holds.

Measured on an MI355X, worst case over the shapes, as a share of the bound (off 1 / its twin at 1): k_step after one step
f 60 % / 48 %, feq 72 % / 60 %, rho 72 % / 72 %, u 4 % / 4 %, v 4 % / 5 % of TOL1; after eleven f 16 % / 14 %, rho 17 % / 15 %,
u 14 % / 12 %, v 6 % / 5 % of contract_tol(11).  Nothing is lost off 1.  One move_bcs call: 13 % of 2.5e-7; the imposed density:
at most 61 % of 4 x 2^-24 rho; the executed reference's fixture: 48 % of TOL1 at step 1; the Cython path after 23 steps: rho 23 %,
u 21 % of its bounds; k_step with the parameter at 1: at least 4.2e-2 away on every one of its cells.

One-line defects tried against this file's 67 cases (none kept; each green without it):
  * `a.rho_out` in both arms of collide_row's out-of-line call (kernels_fused.h)        ->  6 red (every fused kernel, cavity, all
    three widths; with this defect the every-fused-kernel and wall-column tests of test_gpu_edge_obstacles.py stay green);
  * `1.f` for rho0 in the `e && n` closure of bc_cavity_cell (d2q9_cell.h)              -> 24 red (phases, k_step, every fused
    kernel, tiles: every cavity case);
  * `rho = 1.f` for `rho = a.rho_out` in c1_moments (kernels_phases.h)                  -> 12 red (every Cython-path case);
  * `a.rho_out = s->p.inlet_rho` where launch.cpp fills StepArgs                        -> 25 red (every pipe case of the fused
    kernels, the fork and both fixtures included; the phase kernels take PhaseArgs from lb_hip.cpp and stay green).
"""
import numpy as np
import pytest

from conftest import golden
from kernel_variants import assert_forced_kernel, same_bits
from LB_D2Q9.variants import AUTO, K_DEEP2, K_DEEP6, K_DEEP7, K_STEP, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_TILE4, TILES, marching
from test_gpu_edge_obstacles import FIELDS, VARIANTS, bounced, edge_mask, engine, make_pair
from test_gpu_parity import TOL1, TOLN, _random_state, assert_fields_close, contract_tol, maxdiff
from test_oracle_golden import assert_imposed_density

pytestmark = pytest.mark.gpu

PIPE = [(0.9337, 0.93), (1.0743, 1.07)]                # (inlet_rho, outlet_rho)
CAVITY = [(0.06, 0.93), (0.06, 1.07)]                  # (lid_u, rho0)
FORK = (1.0002, 0.9998)                                # (inlet_rho, outlet_rho) of semantics='d2q9i': fluid at 1, amp = 0.001

# (family, the handle's keywords, density of the fluid)
OFF_ONE = [("pipe", dict(inlet_rho=a, outlet_rho=b), b) for a, b in PIPE] + [("cavity", dict(lid_u=a, rho0=b), b) for a, b in CAVITY]
AT_ONE = {"pipe": dict(inlet_rho=1.004, outlet_rho=1.0), "cavity": dict(lid_u=0.06, rho0=1.0)}       # the density-1 twins
IDS = ["%s-%s" % (bc, rho) for bc, _, rho in OFF_ONE]
OMEGA = 1.6                                            # the oracle's stability was checked at it
PHASE_TOL = dict(f=2.5e-7, rho=5e-7, u=1e-6, v=1e-6)   # one phase call (test_gpu_parity.py's header)
NOT_VACUOUS = 1e-2                                     # a fifth of what the oracle measured


def fluid_state(rng, nx, ny, density, amp=0.02):
    return (density * _random_state(rng, nx, ny, amp).astype(np.float64)).astype(np.float32)


def code_of(oracle, bc):
    return {"pipe": oracle.BC_PIPE, "cavity": oracle.BC_CAVITY}[bc]


def param_at_one(kw):
    """The same handle with the one parameter under test put back to 1."""
    return dict(kw, **({"outlet_rho": 1.0} if "outlet_rho" in kw else {"rho0": 1.0}))


def assert_parameter_is_felt(bc, nx, ny, mask, f0, kw, got1):
    """Not vacuous: k_step once with the parameter at 1 on the same state differs from the off-1 run `got1` (fields after ONE
    step) by more than NOT_VACUOUS on f at every cavity corner / at every non-solid cell of the outlet column."""
    s = engine(bc, nx, ny, OMEGA, mask, f0, K_STEP, **param_at_one(kw))
    s.run(1)
    d = np.abs(s.get_fields(("f",))["f"].astype(np.float64) - got1["f"]).max(axis=2)
    s.close()
    if bc == "cavity":
        cells = np.array([d[0, 0], d[0, -1], d[-1, 0], d[-1, -1]])
    else:
        cells = d[-1] if mask is None else d[-1][~mask[-1]]
    assert cells.size and cells.min() > NOT_VACUOUS, (bc, kw, cells.min())
    return float(cells.min())


# ---- a. the phases, one call each -------------------------------------------------------------------------------------------
def _phase_mask(rng, nx, ny, bc):
    """37 x 19: the fixtures' disc (the corners stay fluid); 5 x 7: edge_mask (two corners and an inlet cell solid)"""
    if (nx, ny) == (37, 19):
        return np.asarray(golden("o2_offone_37x19")["mask"], bool)
    return edge_mask(rng, nx, ny, bc)


@pytest.mark.parametrize("nx,ny", [(37, 19), (5, 7)])
@pytest.mark.parametrize("bc,kw,density", OFF_ONE + [("pipe", dict(inlet_rho=FORK[0], outlet_rho=FORK[1], semantics="d2q9i"), 1.0)],
                         ids=IDS + ["d2q9i"])
def test_phases_off_one_vs_oracle(lbhip, oracle, bc, kw, density, nx, ny):
    rng = np.random.default_rng(nx * 1000 + ny)
    fork = kw.get("semantics") == "d2q9i"
    f0 = fluid_state(rng, nx, ny, density, 0.001 if fork else 0.02)
    mask = _phase_mask(rng, nx, ny, bc)
    sim, ref = make_pair(oracle, bc, nx, ny, 1.0 if fork else OMEGA, mask, f0, **kw)
    sim.move_bcs(); ref.move_bcs()
    got = sim.get_fields(("f",))
    print("%s %s %d x %d, move_bcs:" % (bc, kw, nx, ny))
    assert_fields_close(got, ref.get_fields(), dict(f=PHASE_TOL["f"]))
    worst = assert_imposed_density(got["f"], mask, bc, kw.get("inlet_rho"), kw.get("outlet_rho"), kw.get("rho0"))
    print("imposed density: %.0f %% of 4 x 2^-24 rho" % (100 * worst))
    sim.set_f(f0); ref.set_f(f0)
    sim.update_hydro(); ref.update_hydro()
    print("%s %s %d x %d, update_hydro:" % (bc, kw, nx, ny))
    assert_fields_close(sim.get_fields(("rho", "u", "v")), ref.get_fields(), {k: PHASE_TOL[k] for k in ("rho", "u", "v")})
    sim.close()


@pytest.mark.parametrize("nx,ny", [(37, 19), (5, 7)])
@pytest.mark.parametrize("inlet_rho,outlet_rho", PIPE)
def test_cython_phases_off_one_vs_oracle(lbhip, oracle, inlet_rho, outlet_rho, nx, ny):
    """k1_hydro, then k1_bcs fed by the u it stored: the override stores the outlet's density itself, and the rule then closes
    both columns on their densities."""
    from LB_D2Q9.simulation import Simulation
    rng = np.random.default_rng(nx * 1000 + ny + 1)
    f0 = fluid_state(rng, nx, ny, outlet_rho)
    mask = _phase_mask(rng, nx, ny, "pipe")
    sim = Simulation(nx, ny, 1.3, bc="pipe", inlet_rho=inlet_rho, outlet_rho=outlet_rho, obstacle_mask=mask, semantics="cython")
    ref = oracle.O1Sim(nx, ny, 1.3, inlet_rho, outlet_rho, mask=mask, numpy2=False)
    sim.set_f(f0)
    ref.f[...] = f0.transpose(2, 0, 1)
    sim.update_hydro(); ref.update_hydro()
    g = sim.get_fields(("rho", "u", "v"))
    print("cython (%s, %s) %d x %d, update_hydro:" % (inlet_rho, outlet_rho, nx, ny))
    assert_fields_close(g, ref.get_fields(), {k: PHASE_TOL[k] for k in ("rho", "u", "v")})
    assert np.all(g["rho"][-1, :] == np.float32(outlet_rho)) and np.all(g["rho"][0, :] == np.float32(inlet_rho))
    sim.move_bcs(); ref.move_bcs()
    got = sim.get_fields(("f",))
    print("cython (%s, %s) %d x %d, move_bcs:" % (inlet_rho, outlet_rho, nx, ny))
    assert_fields_close(got, dict(f=ref.f.transpose(1, 2, 0)), dict(f=PHASE_TOL["f"]))
    worst = assert_imposed_density(got["f"], mask, "pipe", inlet_rho, outlet_rho)
    print("imposed density: %.0f %% of 4 x 2^-24 rho" % (100 * worst))
    sim.close()


@pytest.mark.parametrize("i", [0, 1])
def test_phases_and_fused_run_vs_executed_reference_off_one(lbhip, i):
    """o2_offone_37x19: D2Q9.cl executed at PIPE[i] (oracle/make_golden.py gen_o2_boundary_densities)."""
    from LB_D2Q9.simulation import Simulation
    d = golden("o2_offone_37x19")
    p = "p%d_" % i
    assert (float(d["inlet_rho"][i]), float(d["outlet_rho"][i])) == PIPE[i]
    m = np.asarray(d["mask"], bool)
    for variant in (K_STEP, AUTO):
        sim = Simulation(int(d["nx"]), int(d["ny"]), float(d["omega"]), bc="pipe", inlet_rho=PIPE[i][0], outlet_rho=PIPE[i][1], obstacle_mask=m)
        sim.set_variant(variant)
        sim.set_f(d[p + "f0"])
        sim.move_bcs()                               # move_bcs + bounceback_in_obstacle: the fixture holds the first
        assert_fields_close(sim.get_fields(("f",)), dict(f=bounced(d[p + "after_bcs_f"], m)), dict(f=PHASE_TOL["f"]))
        sim.set_f(d[p + "f0"])
        sim.update_hydro()
        assert_fields_close(sim.get_fields(("rho", "u", "v")), d, {k: PHASE_TOL[k] for k in ("rho", "u", "v")}, p + "hydro_")
        sim.set_f(d[p + "f0"])
        done = 0
        for n in (1, 10, 50):
            sim.run(n - done)
            done = n
            print("o2_offone_37x19 %s, variant %d, step %d:" % (PIPE[i], variant, n))
            assert_fields_close(sim.get_fields(), d, TOL1 if n == 1 else TOLN, "%ss%d_" % (p, n))
        sim.close()


def test_d2q9i_phases_and_fused_run_vs_executed_fork_off_one(lbhip):
    """o2_d2q9i_offone_37x19: D2Q9i.cl executed at FORK; bounds of test_gpu_d2q9i.py."""
    from LB_D2Q9.simulation import Simulation
    d = golden("o2_d2q9i_offone_37x19")
    assert (float(d["inlet_rho"]), float(d["outlet_rho"])) == FORK
    m = np.asarray(d["mask"], bool)
    for variant in (K_STEP, AUTO):
        sim = Simulation(int(d["nx"]), int(d["ny"]), float(d["omega"]), bc="pipe", inlet_rho=FORK[0], outlet_rho=FORK[1], obstacle_mask=m,
                         semantics="d2q9i")
        sim.set_variant(variant)
        sim.set_f(d["f0"])
        sim.move_bcs()
        assert_fields_close(sim.get_fields(("f",)), dict(f=bounced(d["after_bcs_f"], m)), dict(f=PHASE_TOL["f"]))
        sim.set_f(d["f0"])
        sim.run(1)
        assert_fields_close(sim.get_fields(), d, TOL1, "s1_")
        sim.run(7)
        g = sim.get_fields()
        for k in FIELDS:
            want = d["s8_" + k]
            span = float(np.abs(want - want.mean()).max())
            print("d2q9i fixture, 8 steps, %s: %.2e / %.1e" % (k, maxdiff(g[k], want), max(1e-4 * span, TOLN[k])))
            assert maxdiff(g[k], want) <= max(1e-4 * span, TOLN[k]), k
        sim.close()


# ---- b. k_step against the oracle, with the density-1 twin of every case ------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(3, 3), (5, 7), (256, 3), (67, 29), (130, 130)])
@pytest.mark.parametrize("bc,kw,density", OFF_ONE, ids=IDS)
def test_k_step_off_one_vs_oracle_with_its_twin_at_one(lbhip, oracle, bc, kw, density, nx, ny):
    """One step within TOL1, eleven within contract_tol(11), off 1 and -- same seed, same mask -- at 1: an off-1 case outside
    the bound while its twin passes is a finding about the kernel or the oracle, not a reason to widen anything."""
    for label, k, rho in (("off 1", kw, density), ("at 1", AT_ONE[bc], 1.0)):
        rng = np.random.default_rng(nx * 1000 + ny)
        f0 = fluid_state(rng, nx, ny, rho)
        mask = edge_mask(rng, nx, ny, bc) if (nx, ny) != (3, 3) else None
        sim, ref = make_pair(oracle, bc, nx, ny, OMEGA, mask, f0, **k)
        sim.set_variant(K_STEP)
        sim.run(1); ref.run(1)
        got1 = sim.get_fields()
        print("%s %s %d x %d, %s, 1 step:" % (bc, k, nx, ny, label))
        assert_fields_close(got1, ref.get_fields(), TOL1)
        sim.run(10); ref.run(10)
        print("%s %s %d x %d, %s, 11 steps:" % (bc, k, nx, ny, label))
        assert_fields_close(sim.get_fields(), ref.get_fields(), contract_tol(11))
        sim.close()
        if rho != 1.0:
            print("parameter at 1: min |df| on its cells %.1e" % assert_parameter_is_felt(bc, nx, ny, mask, f0, k, got1))


# ---- c. every fused kernel, bit for bit ------------------------------------------------------------------------------------------
def _every_kernel(oracle, bc, kw, density, nx, ny, variants, first, second, seed):
    rng = np.random.default_rng(seed)
    f0 = fluid_state(rng, nx, ny, density)
    mask = edge_mask(rng, nx, ny, bc)
    assert (~mask[-1]).any() and mask[-1].any()                 # solid and fluid cells on the outlet column
    one = engine(bc, nx, ny, OMEGA, mask, f0, K_STEP, **kw)
    one.run(1)
    assert_parameter_is_felt(bc, nx, ny, mask, f0, kw, one.get_fields(("f",)))
    one.close()
    want = None
    for variant in variants:
        s = engine(bc, nx, ny, OMEGA, mask, f0, variant, **kw)
        if variant != AUTO:
            assert_forced_kernel(s, variant)
        s.run(first)
        s.run(second)
        got = s.get_fields(FIELDS)
        s.close()
        if want is None:
            assert variant == K_STEP
            want = got
        else:
            same_bits(got, want, (bc, kw, nx, ny, variant))
    o = oracle.O2Sim(nx, ny, OMEGA, code_of(oracle, bc), kw.get("inlet_rho", 1.), kw.get("outlet_rho", 1.), kw.get("lid_u", 0.),
                     kw.get("rho0", 1.), mask=mask)
    o.set_f(f0)
    o.run(first + second)
    print("%s %s %d x %d, k_step, %d steps:" % (bc, kw, nx, ny, first + second))
    assert_fields_close(want, o.get_fields(), contract_tol(first + second))


# 513 = 2 x 256 + 1: the outlet column is the one cell past a 256-strip of k_step2 ... k_step4, computed in a halo lane;
# 721 = 3 x 240 + 1: a last strip of k_step5 / k_deep that holds only the outlet column; 960 = 4 x 240: the outlet column is the
# last stored cell of a strip
@pytest.mark.parametrize("nx", [513, 721, 960])
@pytest.mark.parametrize("bc,kw,density", OFF_ONE, ids=IDS)
def test_every_fused_kernel_off_one_bitwise(lbhip, oracle, bc, kw, density, nx):
    _every_kernel(oracle, bc, kw, density, nx, 131, VARIANTS, 12, 7, nx)


@pytest.mark.parametrize("nx,ny", [(96, 64), (130, 70)])
@pytest.mark.parametrize("bc,kw,density", OFF_ONE, ids=IDS)
def test_tile_kernel_and_automatic_choice_off_one_bitwise(lbhip, oracle, bc, kw, density, nx, ny):
    _every_kernel(oracle, bc, kw, density, nx, ny, (K_STEP, K_TILE4, AUTO), 9, 8, 7 * nx + ny)


@pytest.mark.parametrize("nx,ny,masked", [(513, 131, True), (721, 131, False)])
def test_d2q9i_every_fused_kernel_off_one(lbhip, oracle, nx, ny, masked):
    """The variant list and the oracle bound of test_d2q9i_every_fused_kernel_bitwise_and_vs_oracle at FORK."""
    rng = np.random.default_rng(nx + ny)
    f0 = fluid_state(rng, nx, ny, 1.0, amp=0.001)
    mask = edge_mask(rng, nx, ny, "pipe") if masked else None
    kw = dict(inlet_rho=FORK[0], outlet_rho=FORK[1], semantics="d2q9i")
    variants = (K_STEP, K_STEP2, K_STEP3, K_STEP4, marching(4, nt_stores=False) | TILES, K_STEP5, K_DEEP6, K_DEEP7, K_DEEP2)
    outs = []
    for variant in variants:
        s = engine("pipe", nx, ny, 1.0, mask, f0, variant, **kw)
        assert_forced_kernel(s, variant)
        assert "D2Q9i" in s.hot_kernel()
        s.run(5); s.run(3)
        outs.append(s.get_fields(FIELDS))
        s.close()
    for variant, o in zip(variants[1:], outs[1:]):
        same_bits(o, outs[0], (nx, ny, variant))
    ref = oracle.O2Sim(nx, ny, 1.0, oracle.BC_PIPE, FORK[0], FORK[1], mask=mask, d2q9i=True)
    ref.set_f(f0)
    ref.run(8)
    w = ref.get_fields()
    for k in FIELDS:
        span = float(np.abs(w[k] - w[k].mean()).max())
        print("d2q9i %d x %d, 8 steps, %s: %.2e / %.1e" % (nx, ny, k, maxdiff(outs[0][k], w[k]), max(1e-4 * span, TOLN[k])))
        assert maxdiff(outs[0][k], w[k]) <= max(1e-4 * span, TOLN[k]), k


# ---- d. the Cython path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nx,ny,kernel", [(101, 38, "k1_fstep"), (64, 64, "k1_tile4")])      # 64 x 64: the smallest box of LDS tiles
@pytest.mark.parametrize("inlet_rho,outlet_rho", PIPE)
def test_cython_path_off_one_fused_run_equals_phase_calls_and_oracle(lbhip, oracle, inlet_rho, outlet_rho, nx, ny, kernel, masked):
    """As test_cython_path_fused_run_equals_phase_calls, on handles that take outlet_rho (the drop-in classes fix it at 1), and
    against the oracle's float32 mode after the 23 steps within test_gpu_cython_path.py's bounds."""
    from LB_D2Q9.simulation import Simulation
    rng = np.random.default_rng(nx + ny)
    f0 = fluid_state(rng, nx, ny, outlet_rho)
    mask = oracle.disc_mask(nx, ny, nx / 3., ny / 2., ny / 6.) if masked else None

    def handle():
        s = Simulation(nx, ny, 1.3, bc="pipe", inlet_rho=inlet_rho, outlet_rho=outlet_rho, obstacle_mask=mask, semantics="cython")
        s.set_fields(np.full((nx, ny), outlet_rho), np.zeros((nx, ny)), np.zeros((nx, ny)))
        s.set_f(f0)
        return s

    a, b = handle(), handle()
    assert kernel in a.hot_kernel(), a.hot_kernel()
    if kernel == "k1_tile4":
        for smaller in ((63, 64), (64, 63)):
            t = Simulation(smaller[0], smaller[1], 1.3, bc="pipe", semantics="cython")
            assert "k1_fstep" in t.hot_kernel()
            t.close()
    a.run(1); a.run(10); a.run(12)
    for _ in range(23):
        b.move_bcs(); b.move(); b.update_hydro(); b.update_feq(); b.collide_particles()
    ga, gb = a.get_fields(), b.get_fields()
    for k in ("f", "rho", "u", "v", "feq"):
        assert np.array_equal(ga[k], gb[k]), k
    assert np.all(np.isfinite(ga["f"]))
    ref = oracle.O1Sim(nx, ny, 1.3, inlet_rho, outlet_rho, mask=mask, numpy2=False)
    ref.rho[...] = outlet_rho
    ref.f[...] = f0.transpose(2, 0, 1)
    ref.run(23)
    print("cython (%s, %s) %d x %d, masked %s, 23 steps:" % (inlet_rho, outlet_rho, nx, ny, masked))
    assert_fields_close(ga, dict(f=ref.f.transpose(1, 2, 0), rho=ref.rho, u=ref.u, v=ref.v), dict(rho=1e-5, u=5e-6, v=5e-6, f=1e-5))
    assert np.all(ga["rho"][-1, :] == np.float32(outlet_rho))
    a.close(); b.close()
