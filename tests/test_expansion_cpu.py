"""Noisy strains on a shared nutrient, without a GPU: the numpy model against the fixtures recorded from the reference's C (within the
parity contract, the links set to 0 exactly), what the fixtures claim to be, the refusals that need no device, the three ABI symbols,
the drop-in class's constants against the reference's formulas, the package without the library."""
import ctypes as ct
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
from expansion_model import ExpansionModel, from_fixture
from scalar_model import contract_tol

RUN_FIXTURES = ("ex_run_open_37x23", "ex_run_periodic_37x23", "ex_front_21x13", "ex_three_5x4", "ex_one_3x3")
PHASES = "ex_phases_21x13"
ENTRY_POINTS = ("lb_run_expansion", "lb_update_hydro_expansion", "lb_collide_expansion")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def hold(label, n, have, want):
    """Print measured / bound for f and rho, then hold each to the contract's bound; the links that are exactly 0 must be the same."""
    tol = contract_tol(n)
    for k in ("f", "rho"):
        d = maxdiff(have[k], want[k])
        print("%s: %s %.2e / %.1e" % (label, k, d, tol[k]))
        assert d <= tol[k], (label, k, d, tol[k])
    assert np.array_equal(np.asarray(have["f"]) == 0, np.asarray(want["f"]) == 0), label
    assert np.array_equal(np.asarray(have["rho"]) == 0, np.asarray(want["rho"]) == 0), label


@pytest.mark.parametrize("milstein", ("double", "single"))
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_reproduces_the_reference(name, milstein):
    """milstein='single' is the engine's float32 Milstein product: the contract's tolerance covers it."""
    d = golden(name)
    m = from_fixture(d, np.float32, milstein)
    done = 0
    for n in [int(s) for s in d["steps"]]:
        m.run(n - done)
        done = n
        hold("%s after %d (%s)" % (name, n, milstein), n, m.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n]))
    assert m.t == [done] * m.np_


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_float64_twin_stays_with_the_reference(name):
    """The float64 model from the same start and the same float32 normals: the reference's float32 arithmetic drifts from it by no
    more than the contract allows per step, and it sets the same links to 0."""
    d = golden(name)
    m = from_fixture(d, np.float64)
    n = int(d["steps"][0])
    m.run(n)
    hold("%s after %d (float64)" % (name, n), n, m.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n]))


def test_model_reproduces_the_reference_phase_by_phase():
    d = golden(PHASES)
    m = from_fixture(d, np.float32)
    m.noise_fields = [d["z"][0][:, :, i] for i in range(m.np_)]
    tol = contract_tol(1)
    m.move()
    assert np.array_equal(m.get_fields()["f"], d["f_move"], equal_nan=True)
    m.update_hydro()
    assert maxdiff(m.get_fields()["rho"], d["rho_hydro"]) <= tol["rho"]
    assert np.array_equal(m.get_fields()["rho"] == 0, d["rho_hydro"] == 0)
    m.update_feq()
    assert maxdiff(m.get_fields()["feq"], d["feq_feq"]) <= tol["f"]
    zeroed = m.collide_particles()
    assert maxdiff(m.get_fields()["f"], d["f_collide"]) <= tol["f"]
    assert np.array_equal(m.get_fields()["f"] == 0, d["zeroed"])
    assert np.array_equal(zeroed | (m.get_fields()["f"] == 0), d["zeroed"])


def test_fixtures_are_what_they_claim():
    for name in RUN_FIXTURES + (PHASES,):
        d = golden(name)
        nf = len(d["omega"]) + 1
        assert d["f0"].shape == (int(d["nx"]), int(d["ny"]), nf, 9) and d["f0"].dtype == np.float32 and d["f0"].flags.f_contiguous, name
        assert d["z"].shape[1:] == (int(d["nx"]), int(d["ny"]), nf - 1) and len(set(int(s) for s in d["seeds"])) == nf - 1, name
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 1 << 20, name
    for name in ("ex_run_open_37x23", "ex_run_periodic_37x23"):
        d = golden(name)
        cut = float(d["zero_cutoff"])
        assert [int(n) for n in d["steps"]] == [1, 10, 50] and len(d["omega"]) == 2
        assert max(float(np.max(np.abs(d["u"]))), float(np.max(np.abs(d["v"])))) <= float(np.float32(0.07)) and float(np.std(d["u"])) > 0
        assert all(float(d["rho_%d" % n].min()) >= 2 * cut and (d["f_%d" % n] > 0).all() for n in (1, 10, 50)), name
    d = golden("ex_front_21x13")
    assert int(d["edge_zero"]) == 1 and (d["f0"][:, 4:, :2, :] == 0).all() and (d["f0"][:, :, 2, :] > 0).all()
    assert (d["rho_8"][:, :, :2] > 0).sum() > (d["rho_1"][:, :, :2] > 0).sum() and (d["rho_8"][:, :, :2] == 0).any()
    assert (len(golden("ex_three_5x4")["omega"]), len(golden("ex_one_3x3")["omega"])) == (3, 1)
    d = golden(PHASES)
    z = d["zeroed"]
    assert z[1:3, :, 0].all() and z[13:15, :, 2].all() and z[9:11, 2:-2, 1].all() and not z[17:].any() and np.isnan(d["f0"]).any()
    assert (d["rho_hydro"][5:7, :, 0] > 0).all() and z[5:7, 1:-1, 0].any(axis=2).all() and float(d["z"][0][5:7, :, 0].max()) <= -4.


def test_collision_conserves_strains_plus_nutrient_while_no_floor_fires():
    d = golden("ex_run_periodic_37x23")
    m = from_fixture(d, np.float64)
    total = lambda: float(m.get_fields()["f"].sum())
    before = total()
    for _ in range(5):
        assert not m.step().any()
    assert abs(total() - before) <= 1e-10 * before


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_bound_and_refuse_null(lbhip):
    from LB_D2Q9 import _native
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    for name in ENTRY_POINTS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and name in _native.SIGNATURES and fn.argtypes is not None, name
        assert re.search(r"\bint %s\(lb_sim \*\*fields, int count, const lb_expansion_params \*p" % name, text), name
        args = [0 if a in (ct.c_int, ct.c_float) else None for a in fn.argtypes]
        assert fn(*args) == -1 and b"null handle array" in lbhip.lb_last_error(), name
    assert len(_native.SIGNATURES["lb_run_expansion"][0]) == 4 and len(_native.SIGNATURES["lb_collide_expansion"][0]) == 3
    m = re.search(r"typedef struct \{ float (\w+); \} lb_expansion_params;", text)
    assert m and [m.group(1)] == [n for n, _ in _native.ExpansionParams._fields_] and ct.sizeof(_native.ExpansionParams) == 4


def test_refusals_that_need_no_device(lbhip):
    """LB_ERR_ARG (-1) with the reason, before any device is touched: a null array, null parameters, a count outside 2 ... 4, a null
    handle, a member that is no scalar lattice on the GPU (a handle of the CPU backend), all three calls alike."""
    from LB_D2Q9 import _native
    from LB_D2Q9.simulation import Simulation
    p = ct.byref(_native.ExpansionParams(0.01))
    nulls = (ct.c_void_p * 4)()
    for name in ENTRY_POINTS:
        fn = getattr(lbhip, name)
        tail = (3,) if name == "lb_run_expansion" else ()
        assert fn(nulls, 2, None, *tail) == -1 and b"null parameters" in lbhip.lb_last_error(), name
        for count in (-1, 0, 1, 5):
            assert fn(nulls, count, p, *tail) == -1 and b"takes 2..4 handles" in lbhip.lb_last_error(), (name, count)
        assert fn(nulls, 3, p, *tail) == -1 and b"null handle in the set" in lbhip.lb_last_error(), name
        host = Simulation(8, 6, 1.0, semantics="cython", device=_native.LB_DEVICE_CPU)
        try:
            pair = (ct.c_void_p * 2)(host._h, host._h)
            assert fn(pair, 2, p, *tail) == -1 and b"handle 0 is not a scalar lattice on the GPU" in lbhip.lb_last_error(), name
        finally:
            host.close()


def test_build_lists_the_unit():
    build = open(os.path.join(ROOT, "2d-lb_amd", "build.py")).read()
    assert '"expansion.cpp"' in build


# ---- the Python side without the engine ---------------------------------------------------------------------------------------------
class _NoEngine(object):
    MAX_STRAINS = 3

    def __init__(self, *args, **kw):
        self.args, self.kw, self.calls = args, kw, []

    def get_edge_state(self):
        return np.zeros((3, 0), np.float32)

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, a, kw))


def reference_constants(mu_list, D_list, mu_standard, D_standard, Nb, Dc, time_prefactor, N, Lx, Ly):
    """set_characteristic_length_time, set_field_constants and initialize_grid_dims, restated line by line."""
    cs = np.float32(1. / np.sqrt(3))
    mu, D = np.array(mu_list, np.float64), np.array(D_list, np.float64)
    L, T = 2 * np.sqrt(D_standard / mu_standard), 1. / mu_standard
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    lb_D = ((1. / (4. * D_standard)) * D * (delta_t / delta_x ** 2)).astype(np.float32)
    lb_D_n = Dc / (4 * D_standard) * (delta_t / delta_x ** 2)
    return dict(L=L, T=T, vf=L / T, delta_x=delta_x, delta_t=delta_t, ulb=delta_t / delta_x,
                lb_G=((mu / mu_standard) * delta_t).astype(np.float32),
                lb_Dg=((mu / Nb) * (1. / (4 * D_standard)) * delta_t).astype(np.float32),
                lb_D_population=lb_D, omega=((.5 + lb_D / cs ** 2) ** -1.).astype(np.float32),
                omega_nutrient=np.float32((.5 + lb_D_n / np.float64(cs ** 2)) ** -1.),
                nx=N * int(Lx / L) + 2, ny=N * int(Ly / L) + 2)


@pytest.mark.parametrize("kw", (
    dict(Lx=4., Ly=6., vx=0., vy=0., vc=0., mu_standard=1., mu_list=[1., 1.1], D_standard=1., D_list=[1., 0.8], Nb=10., Dc=1., N=10),
    dict(Lx=3., Ly=2.5, vx=0.3, vy=-0.2, vc=0.5, mu_standard=2., mu_list=[2., 1.5, 2.5], D_standard=0.5, D_list=[0.5, 0.6, 0.4], Nb=40.,
         Dc=2., time_prefactor=0.8, N=12, zero_cutoff=0.005, seed=7, bc="periodic"),
))
def test_dropin_constants_with_the_engine_away(monkeypatch, kw):
    from LB_D2Q9.advecting_range_expansion import stochastic_nutrients as sn
    monkeypatch.setattr(sn, "Expansion_Set", _NoEngine)
    sim = sn.Expansion(two_d_local_size=(16, 16), use_interop=True, **kw)
    want = reference_constants(kw["mu_list"], kw["D_list"], kw["mu_standard"], kw["D_standard"], kw["Nb"], kw["Dc"],
                               kw.get("time_prefactor", 1.), kw["N"], kw["Lx"], kw["Ly"])
    for k, v in want.items():
        got = getattr(sim, k)
        assert np.array_equal(np.asarray(got), np.asarray(v)) and np.asarray(got).dtype == np.asarray(v).dtype or k in ("nx", "ny") and int(got) == v, (k, got, v)
    assert isinstance(sim.nx, np.int32) and int(sim.num_populations) == len(kw["mu_list"]) and sim.zero_cutoff == np.float32(kw.get("zero_cutoff", 0.01))
    e = sim.sim
    assert e.args[:2] == (sim.nx, sim.ny) and e.kw["bc"] == kw.get("bc", "open") and e.kw["zero_cutoff"] == sim.zero_cutoff
    name, a, _ = e.calls[0]
    assert name == "set_noise" and np.array_equal(a[0], sim.lb_Dg) and a[1] == kw.get("seed", 0)
    rho = [c for c in e.calls if c[0] == "set_fields"][0][1][0]
    assert rho.shape == (sim.nx, sim.ny, len(kw["mu_list"]) + 1) and (rho[:, 2 * kw["N"]:, :-1] == 0).all()
    assert np.allclose(rho[:, :2 * kw["N"], :-1], 1. / len(kw["mu_list"])) and (rho[:, :, -1] == 1).all()
    u = [c for c in e.calls if c[0] == "set_fields"][0][1][1]
    if kw["vc"] == 0:
        assert (u == 0).all()
    else:
        assert np.allclose(u, want["ulb"] * (kw["vc"] / want["vf"]) * kw["vx"] / kw["vc"])
    assert [c[0] for c in e.calls if c[0] in ("init_pop", "set_edge_state")] == ["init_pop", "set_edge_state"]
    for name in ("init_hydro", "update_feq", "init_f", "move", "move_bcs", "update_hydro", "collide_particles", "run", "get_fields",
                 "get_nondim_fields", "get_physical_fields"):
        assert callable(getattr(sim, name)), name


def test_dropin_refuses_what_is_not_built(monkeypatch):
    from LB_D2Q9.advecting_range_expansion import stochastic_nutrients as sn
    monkeypatch.setattr(sn, "Expansion_Set", _NoEngine)
    with pytest.raises(ValueError, match="at most 3 strains"):
        sn.Expansion(mu_list=[1.] * 4, D_list=[1.] * 4)
    with pytest.raises(ValueError, match="D_list is required"):
        sn.Expansion(mu_list=[1.])


def test_engine_is_built_on_the_shared_bases():
    from LB_D2Q9 import coupled, expansion_set
    assert issubclass(expansion_set.Expansion_Set, coupled._Lattice_Set) and issubclass(expansion_set.Expansion_Set, coupled._Shared_Velocity)


def test_package_imports_without_the_library(tmp_path):
    """A fresh interpreter with LB_LIB pointing nowhere: the modules import, the parameter arithmetic works; only a handle needs it."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from LB_D2Q9 import expansion_set\n"
            "from LB_D2Q9.advecting_range_expansion import stochastic_nutrients as sn\n"
            "p = sn.expansion_parameters(Lx=4., Ly=4., mu_list=[1.], D_list=[1.], N=10)\n"
            "assert (int(p['nx']), int(p['ny'])) == (22, 22)\n"
            "print('ok')\n" % os.path.join(ROOT, "2d-lb_amd"))
    env = dict(os.environ, LB_LIB=str(tmp_path / "missing.so"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
