"""Surfactant-propelled colonies without a GPU: the numpy model against the fixtures recorded from the reference's C (float64 to
rounding, float32 within the parity contract), what the fixtures claim to be, the drop-in classes' derived constants, the new
ABI symbols and the parameter struct, lb_create's refusals, the launch planner's answers."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from rocket_model import CS32, PARAMS, RocketModel, from_fixture, rocket_bounds
from scalar_model import contract_tol

RUN_FIXTURES = ("ry_flow_37x23", "ry_forces_37x23", "ry_flow_5x4", "ry_flow_3x3")
PHASE_FIXTURES = ("ry_phases_21x13", "ry_forces_phases_21x13")
STEPS = {"ry_flow_37x23": [1, 10, 50, 100], "ry_forces_37x23": [1, 10, 50, 100], "ry_flow_5x4": [1, 10], "ry_flow_3x3": [1, 10]}
NAMES = ("f", "feq", "rho", "u", "v", "op", "Fx", "Fy", "Sx", "Sy")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def bounds(m, n, rho_max):
    """The parity contract for n steps (tests/scalar_model.py) in f, feq, rho, u, v; psi / S and the forces take the bounds that
    follow from rho's through the stencil (rocket_model.rocket_bounds)."""
    tol = contract_tol(n)
    rb = rocket_bounds(m.mode, m.params, rho_max, tol["rho"])
    return dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], op=rb["op"], Fx=rb["F"], Fy=rb["F"], Sx=rb["S"], Sy=rb["S"])


def compare(label, m, n, have, want, which=None, rho_max=None):
    """Print measured / bound for every array, then hold each to its bound."""
    b = bounds(m, n, float(np.max(want["rho"])) if rho_max is None else rho_max)
    for k in [k for k in (which or NAMES) if k in want and k in have]:
        d = maxdiff(have[k], want[k])
        print("%s: %s %.2e / %.1e" % (label, k, d, b[k]))
        assert d <= b[k], (label, k, d, b[k])


def state(m):
    g = m.get_fields()
    if m.mode == "flow":
        g.pop("Sx"), g.pop("Sy")
    return g


def recorded(d, n, tag=""):
    return {k: d["%s_%d%s" % (k, n, tag)] for k in NAMES if "%s_%d%s" % (k, n, tag) in d.files}


def writes(mode, stage):
    if stage == "update_forces":
        return ("op", "Fx", "Fy") + (("Sx", "Sy") if mode == "forces" else ())
    return dict(move=("f",), update_hydro=("rho",), update_velocity=("u", "v"), update_feq=("feq",), collide=("f",))[stage]


# ---- the model against the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_reproduces_the_reference(name):
    d = golden(name)
    assert [int(n) for n in d["steps"]] == STEPS[name]
    m64, m32 = from_fixture(d, np.float64), from_fixture(d, np.float32)
    done = 0
    for n in d["steps"]:
        m64.run(n - done)
        m32.run(n - done)
        done = int(n)
        want = recorded(d, n)
        assert {"rho", "u", "v", "op", "Fx", "Fy"} <= set(want) and ("f" in want) == (n in (d["steps"][0], d["steps"][-1]))
        for k, a in want.items():
            assert maxdiff(getattr(m64, k), a) <= 1e-12, (name, k, n)
        compare("%s step %d, float32 model / reference" % (name, n), m32, n, state(m32), want)
        compare("%s step %d, float32 model / reference's float32 build" % (name, n), m32, n, state(m32), recorded(d, n, "_f32"),
                rho_max=float(want["rho"].max()))


@pytest.mark.parametrize("name", PHASE_FIXTURES)
def test_model_reproduces_the_reference_stage_by_stage(name):
    """... the floored links included: the only place where the floor at 0 and the rho_p > 1 cut-off act."""
    d = golden(name)
    m64, m32 = from_fixture(d, np.float64), from_fixture(d, np.float32)
    assert m64.params["epsilon"] == 2.
    rho_max = float(d["rho_after_update_hydro"].max())
    for stage in m64.STAGES:
        for m in (m64, m32):
            getattr(m, stage)()
        want = {k: d["%s_after_%s" % (k, stage)] for k in writes(m64.mode, stage)}
        for k, a in want.items():
            assert maxdiff(getattr(m64, k), a) <= 1e-12, (stage, k)
        compare("%s after %s" % (name, stage), m32, 1, state(m32) if stage != "update_feq" else dict(feq=m32.feq), want, rho_max=rho_max)
    for m in (m64, m32):
        assert np.array_equal(m.clamped, d["clamped"])
    assert d["clamped"].sum() >= 0.01 * d["clamped"].size
    assert np.array_equal(d["f_after_collide"][:, :, 0, :] == 0, d["clamped"]) and np.array_equal(d["f_after_collide_f32"][:, :, 0, :] == 0, d["clamped"])
    if m64.mode == "forces":                        # the cut-off: cells denser than 1 exist and did not grow
        assert (d["rho_after_update_hydro"][:, :, 0] > 1).sum() > 10


# ---- the fixtures are what they claim to be ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fixture_is_what_it_claims(name):
    """The recorder's acceptance conditions, re-checked on the file: the reference's own float32 build within the contract of its
    float64 build; the start is a float32 droplet at equilibrium without surfactant."""
    d = golden(name)
    m = from_fixture(d, np.float64)
    for n in d["steps"]:
        want, have = recorded(d, n), recorded(d, n, "_f32")
        assert set(have) == set(want) - ({"f"} if n != d["steps"][-1] else set())
        compare("%s f32 build, step %d" % (name, n), m, n, have, want, which=list(have))
        assert np.isfinite(want["rho"]).all()
    f0 = d["f0"]
    assert f0.dtype == np.float32 and f0.shape == (int(d["nx"]), int(d["ny"]), 2, 9) and not f0[:, :, 1].any()
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    assert maxdiff(f0[:, :, 0], w * f0[:, :, 0].astype(np.float64).sum(axis=2, keepdims=True)) < 2e-7


def test_fixture_sizes():
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n))
    largest = max(size(n) for n in os.listdir(os.path.join(ROOT, "tests", "golden")) if not n.startswith("ry_"))
    for n in RUN_FIXTURES + PHASE_FIXTURES:
        assert size(n + ".npz") <= largest, n


# ---- closed forms, float64 model -----------------------------------------------------------------------------------------------
def test_uniform_state_has_no_flow_and_grows_logistically():
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    for mode in ("flow", "forces"):
        m = RocketModel(7, 5, 0.8, 0.9, mode, np.float64, G=0.01, G_c=0.02, epsilon=1., rho_o=1., G_chen=-1., c_o=0.25, alpha=2.)
        m.set_f(w[None, None, None, :] * np.array([0.5, 0.3])[None, None, :, None] * np.ones((7, 5, 2, 9)))
        m.step()
        assert np.abs(m.u).max() < 1e-15 and np.abs(m.Fx).max() < 1e-15
        G, G_c = float(np.float32(0.01)), float(np.float32(0.02))         # (the parameters are float32 values)
        assert np.abs(m.f[:, :, 0].sum(axis=2) - (0.5 + G * 0.5 * 0.5)).max() < 1e-14
        assert np.abs(m.f[:, :, 1].sum(axis=2) - (0.3 + G_c * 0.5)).max() < 1e-14


def test_stencil_is_the_gradient_over_three():
    """grad_w of a linear ramp (away from the wrap) is slope cs^2: u = -epsilon (1 / cs^2) grad_w rho_c = -epsilon slope."""
    m = RocketModel(12, 9, 0.8, 0.8, "flow", np.float64, epsilon=1.5)
    x = np.arange(12.)[:, None] * np.ones((1, 9))
    m.rho[:, :, 1] = 0.01 * x
    m.update_velocity()
    assert np.abs(m.u[2:-2] + 1.5 * 0.01 * (1. / 3.) * float(m.inv_cs2)).max() < 1e-15 and np.abs(m.v[2:-2]).max() < 1e-15


# ---- the drop-in classes' constants ------------------------------------------------------------------------------------------
def restated_constants(mode, N, Lx, Ly, time_prefactor, Dc, Gc):
    """The reference's expressions (rocket_yeast.py:84-142), every operation in the precision the reference's numpy gives it: a
    float32 scalar combined with a Python number is a float64."""
    f32, f64 = np.float32, np.float64
    cs2 = f64(CS32) ** 2
    dx = 1. / N
    if mode == "forces":
        dx = f64(f32(dx))
    dt = time_prefactor * dx ** 2
    if mode == "forces":
        dt = f64(f32(dt))
    lb_D = f32(0.25 * (dt / dx ** 2))
    lb_Dc = f32((0.25 * f64(f32(Dc))) * (dt / dx ** 2))
    return dict(delta_x=dx, delta_t=dt, lb_D=lb_D, lb_Dc=lb_Dc, omega=f32((.5 + f64(lb_D) / cs2) ** -1.), omega_c=f32((.5 + f64(lb_Dc) / cs2) ** -1.),
                lb_G=f32(dt), lb_Gc=f32(f64(f32(Gc)) * dt), nx=int(np.round(N * Lx)), ny=int(np.round(N * Ly)),
                ulb=dt / dx if mode == "flow" else f32(dt) / f32(dx))     # (two float32 scalars: a float32)


class _NoEngine(object):
    """stands in for Surfactant_Colony: the constants are derived before any handle exists"""

    def __init__(self, *a, **kw):
        self.args, self.kw, self.params = a, kw, {}

    def set_params(self, **kw):
        self.params.update(kw)

    def __getattr__(self, name):
        return lambda *a, **kw: None


@pytest.mark.parametrize("kw", [dict(N=10, Lx=3.7, Ly=2.3, Dc=1., Gc=2.), dict(N=7, Lx=1.3, Ly=2.9, Dc=0.3, Gc=1.7, time_prefactor=0.7),
                                dict(N=3, Lx=1., Ly=1., Dc=0.25, Gc=2.), dict(N=13, Lx=2., Ly=1., Dc=2.2, Gc=0.1, time_prefactor=1.3)])
@pytest.mark.parametrize("mode", ("flow", "forces"))
def test_dropin_constants_are_the_references(monkeypatch, mode, kw):
    from LB_D2Q9.rocket_yeast import rocket_yeast, rocket_yeast_forces_only
    monkeypatch.setattr(rocket_yeast, "Surfactant_Colony", _NoEngine)
    cls = rocket_yeast.Rocket_Yeast if mode == "flow" else rocket_yeast_forces_only.Rocket_Yeast_Forces_Only
    sim = cls(rng=3, **kw)
    want = restated_constants(mode, kw["N"], kw["Lx"], kw["Ly"], kw.get("time_prefactor", 1.), kw["Dc"], kw["Gc"])
    for k, v in want.items():
        have = getattr(sim, k)
        assert have == v and (not isinstance(v, np.float32) or isinstance(have, np.float32)), (k, have, v)
    assert (type(sim.delta_x) is np.float32) == (mode == "forces")
    e = sim.engine
    assert e.args == (want["nx"], want["ny"], want["omega"], want["omega_c"]) and e.kw["mode"] == mode
    assert e.params["G"] == want["lb_G"] and e.params["G_c"] == want["lb_Gc"] and ("c_o" in e.params) == (mode == "forces")
    assert rocket_yeast.cs == CS32 and rocket_yeast.w.dtype == np.float32
    for name in ("redo_initial_condition", "update_feq", "init_pop", "move_bcs", "move", "update_u_and_v", "update_hydro",
                 "collide_particles", "run", "update_forces" if mode == "forces" else "update_force"):
        assert callable(getattr(sim, name)), name


def test_reference_defaults_at_N10_are_the_fixtures_parameters():
    """Class defaults at N = 10 with Dc = 1: omega = omega_c = 0.8, lb_G = 0.01, lb_Gc = 0.02 -- the header of the run fixtures."""
    for name, mode in (("ry_flow_37x23", "flow"), ("ry_forces_37x23", "forces")):
        d = golden(name)
        c = restated_constants(mode, 10, 3.7, 2.3, 1., 1., 2.)
        assert (int(d["nx"]), int(d["ny"])) == (c["nx"], c["ny"]) == (37, 23) and str(d["mode"]) == mode
        assert np.array_equal(d["omega"].astype(np.float32), [c["omega"], c["omega_c"]])
        want = dict(G=c["lb_G"], G_c=c["lb_Gc"], epsilon=1., rho_o=1., G_chen=-1., c_o=0.25, alpha=2.)
        assert np.array_equal(d["params"].astype(np.float32), np.array([want[k] for k in PARAMS], np.float32))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_set_rocket", "lb_get_rocket", "lb_run_rocket", "lb_update_velocity_rocket", "lb_update_forces_rocket",
               "lb_collide_rocket", "lb_get_rocket_fields")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION and ct.sizeof(_native.LbParams) == 64
    assert _native.LB_SEM_ROCKET == 11 and (_native.LB_ROCKET_FLOW, _native.LB_ROCKET_FORCES) == (0, 1)
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"\bLB_SEM_ROCKET = 11\b", text) and re.search(r"LB_ROCKET_FLOW = 0, LB_ROCKET_FORCES = 1", text)
    for name in NEW_SYMBOLS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None and re.search(r"\bint %s\(" % name, text), name
        args = [None] + [0 if a is ct.c_int else None for a in fn.argtypes[1:]]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error(), name      # a null handle: an argument error, not a crash
    consts = open(os.path.join(ROOT, "2d-lb_amd", "csrc", "plan_consts.h")).read()
    assert int(re.search(r"constexpr int RY_ROWS = (\d+);", consts).group(1)) == _native.RY_ROWS


def test_rocket_params_struct_round_trip():
    """The binding's struct is the header's, field for field, and keeps float32 values bit for bit."""
    from LB_D2Q9 import _native
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} lb_rocket_params;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), ct.c_int32 if ctype == "int32_t" else ct.c_float) for n in names.split(",")]
    assert fields == list(_native.RocketParams._fields_) and ct.sizeof(_native.RocketParams) == 32
    assert [n for n, _ in fields][1:] == list(PARAMS)
    vals = [np.float32(v) for v in (0.01, 0.02, 1.5, 0.9, -1.25, 0.25, 2.)]
    p = _native.RocketParams(_native.LB_ROCKET_FORCES, *vals)
    q = _native.RocketParams.from_buffer_copy(bytes(p))
    assert q.mode == 1 and [np.float32(getattr(q, k)) for k in PARAMS] == vals
    assert np.frombuffer(bytes(p), np.float32)[1:].tolist() == [float(v) for v in vals]


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 0.8
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_ROCKET, _native.LB_BC_PERIODIC, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(device=-1), b"CPU"),                                      # LB_DEVICE_CPU: refused by name, before any device is touched
    (dict(bc_mode=0), b"LB_BC_PERIODIC only"),                      # every other family with this semantics
    (dict(bc_mode=2), b"LB_BC_PERIODIC only"),
    (dict(bc_mode=3), b"LB_BC_PERIODIC only"),
    (dict(bc_mode=4), b"LB_BC_PERIODIC only"),
    (dict(bc_mode=5), b"LB_BC_PERIODIC only"),
    (dict(bc_mode=6), b"LB_BC_DIRICHLET exists"),
    (dict(bc_mode=7), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(bc_mode=8), b"unknown bc_mode"),
    (dict(nx=2), b"at least 3x3"),
    (dict(ny=2, local_ny=2), b"at least 3x3"),
    (dict(local_ny=6), b"slab"),
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),
    (dict(omega=2.5), b"omega"),
    (dict(reserved=(ct.c_int32 * 1)(1)), b"reserved"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg
    if b"exists" not in word and b"unknown" not in word and b"omega" not in word and b"reserved" not in word:
        assert b"LB_SEM_ROCKET" in msg, msg


# ---- the planner -----------------------------------------------------------------------------------------------------------
PLAN_DRIVER = r"""
#include <stdio.h>
#include "plan.h"
int main()
{
    PlanInputs s;
    s.p = lb_params();
    s.p.nx = 512; s.p.ny = 512; s.p.local_ny = 512; s.p.semantics = LB_SEM_ROCKET; s.p.bc_mode = LB_BC_PERIODIC; s.p.omega = 1.f;
    s.H = 512; s.pitch = 512; s.rowp = 9 * 512; s.plane = 512;
    const int variants[3] = {-1, 0, 1};
    for (int v : variants) {
        s.variant = v;
        int d[32];
        const int c = plan_launches(&s, 5, d, 32);
        for (int i = 0; i < c; ++i) printf("%d ", d[i]);
        char name[512];
        hot_kernel(&s, name, sizeof(name));
        printf("| %d %d %d %d | %s\n", steps_per_launch(&s), rocket_one_launch(&s) ? 1 : 0, scalar_use_tiles(&s) ? 1 : 0, RY_ROWS, name);
    }
    return 0;
}
"""


def test_the_planners_answers_for_both_variants(tmp_path):
    """plan.cpp is plain C++: compiled here with the host compiler.  A colony runs one step per launch in either form, never the
    scalar lattice's tiles; -1 is the one-launch form."""
    from LB_D2Q9 import _native
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    csrc = os.path.join(ROOT, "2d-lb_amd", "csrc")
    (tmp_path / "drv.cpp").write_text(PLAN_DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I" + csrc, str(tmp_path / "drv.cpp"), os.path.join(csrc, "plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode().splitlines()
    rows = "%d" % _native.RY_ROWS
    for line, one in zip(out, (1, 0, 1)):
        steps, answers, name = [x.strip() for x in line.split("|")]
        assert steps == "1 1 1 1 1" and answers == "1 %d 0 %s" % (one, rows), line
        assert name.startswith("k_ry_step (" if one else "k_ry_moments + k_ry_collide (") and name.endswith("<PERIODIC>"), name
        assert ("the %s owned rows" % rows in name) == bool(one)
