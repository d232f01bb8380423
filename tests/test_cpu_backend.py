"""The product's CPU backend (lb_create with device = LB_DEVICE_CPU; 2d-lb_amd/csrc/cpu_backend.h): the reference's CPU class
(cython_dim.pyx Pipe_Flow / Pipe_Flow_Cylinder) behind the same C ABI, on a box without a GPU.  Held DIRECTLY to the fixtures
the imported, cythonized reference produced (tests/golden/o1_*.npz, generator: oracle/make_golden.py) -- not to the oracle, which
the product never touches -- and to BASELINE.json's first configuration (256 x 256 Poiseuille flow, 1000 steps, "CPU path,
no GPU").  u, v are float64 in the reference and inside the backend, float32 across the C ABI: they are compared after
rounding the fixture to float32; f, feq, rho (float32 in the reference) bit for bit."""
import numpy as np
import pytest

from conftest import golden
from test_config1 import KW, STEPS, check_against_reference_fixture, md, startup_profile
from test_oracle_golden import kwargs_of


def f32(a):
    return np.asarray(a).astype(np.float32)


def same_fields(g, d, prefix):
    for k in ("f", "feq", "rho"):
        assert np.array_equal(g[k], d[prefix + k]), (prefix, k)
    for k in ("u", "v"):
        assert np.array_equal(f32(g[k]), f32(d[prefix + k])), (prefix, k)


def test_cpu_backend_pipe_trace_and_runs_bit_exact(lbhip):
    """The imported reference's own run of a 33 x 17 pipe: initial state, the state before its third step, each of the five
    phases of that step, then 50 and 500 steps."""
    from LB_D2Q9.dimensionless import cython_dim as lb
    d = golden("o1_pipe_33x17")
    sim = lb.Pipe_Flow(device=-1, verbose=False, **kwargs_of(d))
    assert (sim.nx, sim.ny) == (int(d["nx"]), int(d["ny"]))
    assert sim.omega == float(d["omega"]) and sim.inlet_rho == float(d["inlet_rho"]) and sim.Re == float(d["Re"])
    assert "cpu backend" in sim._sim.hot_kernel() and sim._sim.steps_per_launch() == 1
    assert np.array_equal(sim.get_fields()["rho"], d["rho0"])
    sim.set_f(d["f0"])                                     # (the reference's own random perturbation of feq)
    sim.run(2)
    same_fields(sim.get_fields(), d, "pre_")
    sim.move_bcs();          assert np.array_equal(sim.get_fields()["f"], d["t_bcs_f"])
    sim.move();              assert np.array_equal(sim.get_fields()["f"], d["t_move_f"])
    sim.update_hydro()
    g = sim.get_fields()
    assert np.array_equal(g["rho"], d["t_hydro_rho"])
    assert np.array_equal(f32(g["u"]), f32(d["t_hydro_u"])) and np.array_equal(f32(g["v"]), f32(d["t_hydro_v"]))
    sim.update_feq();        assert np.array_equal(sim.get_fields()["feq"], d["t_feq"])
    sim.collide_particles(); assert np.array_equal(sim.get_fields()["f"], d["t_collide_f"])
    done = 3
    for n in (50, 500):
        sim.run(n - done)
        done = n
        same_fields(sim.get_fields(), d, "s%d_" % n)


def test_cpu_backend_cylinder_bit_exact(lbhip):
    from LB_D2Q9.dimensionless import cython_dim as lb
    d = golden("o1_cyl_61x41")
    sim = lb.Pipe_Flow_Cylinder(cylinder_center=list(d["cylinder_center"]), cylinder_radius=float(d["cylinder_radius"]),
                                device=-1, verbose=False, **kwargs_of(d))
    assert np.array_equal(np.asarray(sim.obstacle_mask, bool), d["mask"])
    sim.set_f(d["f0"])
    done = 0
    for n in (1, 50, 300):
        sim.run(n - done)
        done = n
        g = sim.get_fields()
        same_fields(g, d, "s%d_" % n)
        assert np.all(g["u"][d["mask"]] == 0)


@pytest.mark.parametrize("name,edge", [("o1_edge_cyl_61x41", "south"), ("o1_edge_cyl_inlet_61x41", "inlet")])
def test_cpu_backend_cylinder_on_the_boundary_bit_exact(lbhip, name, edge):
    """The same cylinder with five of its cells on the south wall row / on the inlet column: the boundary rule and the
    bounce-back on one cell (c1_bcs_cell takes `solid` inside the rule)."""
    from LB_D2Q9.dimensionless import cython_dim as lb
    d = golden(name)
    sim = lb.Pipe_Flow_Cylinder(cylinder_center=list(d["cylinder_center"]), cylinder_radius=float(d["cylinder_radius"]),
                                device=-1, verbose=False, **kwargs_of(d))
    assert np.array_equal(np.asarray(sim.obstacle_mask, bool), d["mask"])
    assert int((d["mask"][:, 0] if edge == "south" else d["mask"][0, :]).sum()) == 5
    sim.set_f(d["f0"])
    done = 0
    for n in (1, 50, 300):
        sim.run(n - done)
        done = n
        g = sim.get_fields()
        same_fields(g, d, "s%d_" % n)
        assert np.all(g["u"][d["mask"]] == 0) and np.all(g["v"][d["mask"]] == 0)


@pytest.mark.parametrize("inlet_rho,outlet_rho", [(0.9337, 0.93), (1.0743, 1.07)])
@pytest.mark.parametrize("nx,ny,masked", [(33, 17, False), (5, 4, False), (3, 3, False), (61, 41, True)])
def test_cpu_backend_boundary_densities_off_one_vs_oracle(lbhip, oracle, inlet_rho, outlet_rho, nx, ny, masked):
    """outlet_rho != 1 and a fluid at that density (the reference's classes always set outlet_rho = 1, and so do the fixtures
    above): against the oracle's restatement of the Cython path, which those fixtures pin bit for bit.  The moment override
    stores the outlet's density itself."""
    from LB_D2Q9.simulation import Simulation
    rng = np.random.default_rng(nx * 100 + ny)
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    # the fluid at rest at the outlet's density, perturbed as the reference's init_pop does: one draw per cell, 0.1 %
    f0 = (outlet_rho * w[None, None, :] * (1 + 0.001 * rng.standard_normal((nx, ny, 1)))).astype(np.float32)
    mask = None
    if masked:
        mask = rng.random((nx, ny)) < 0.05
    # (omega 1.3: at 1.6 this path's plain bounce-back walls drive the 3 x 3 box to NaN within 50 steps, in the oracle as here)
    sim = Simulation(nx, ny, 1.3, bc="pipe", inlet_rho=inlet_rho, outlet_rho=outlet_rho, obstacle_mask=mask,
                     semantics="cython", device=-1)
    ref = oracle.O1Sim(nx, ny, 1.3, inlet_rho, outlet_rho, mask=mask)
    sim.set_f(f0)
    ref.f[...] = f0.transpose(2, 0, 1)
    done = 0
    for n in (1, 5, 50):
        sim.run(n - done); ref.run(n - done)
        done = n
        g = sim.get_fields()
        got = dict(f=g["f"].transpose(2, 0, 1), feq=g["feq"].transpose(2, 0, 1), rho=g["rho"], u=g["u"], v=g["v"])
        same_fields(got, ref.get_fields(), "")
        assert np.all(g["rho"][-1, :] == np.float32(outlet_rho)) and np.all(g["rho"][0, :] == np.float32(inlet_rho))
        print("step %d: max |u| %.3f, rho %.3f ... %.3f" % (n, np.abs(g["u"]).max(), g["rho"].min(), g["rho"].max()))
        assert np.all(np.isfinite(g["f"])) and g["rho"].min() > 0.9 and g["rho"].max() < 1.1       # (w_k rho stays in w_k's binade)
    sim.close()


def test_config1_256_poiseuille_on_the_cpu_backend_without_a_gpu(lbhip):
    """BASELINE.json configs[0] -- 256 x 256 Poiseuille pipe flow on the CPU path, no GPU -- through the product: 1000 steps from
    f = feq against the imported reference's own run of that case (rows / columns / means stored in o1_config1_256; rho bit for
    bit, u and v to the float32 rounding of the ABI) and the analytic start-up profile."""
    from LB_D2Q9.dimensionless import cython_dim as lb
    d = golden("o1_config1_256")
    assert dict(zip(d["kw_names"], d["kw_vals"])) == KW and int(d["steps"]) == STEPS
    sim = lb.Pipe_Flow(device=-1, verbose=False, **KW)
    assert (sim.nx, sim.ny) == (256, 256)
    assert sim.omega == float(d["omega"]) and sim.inlet_rho == float(d["inlet_rho"])
    sim.init_pop(amplitude=0.)
    sim.run(STEPS)
    g = sim.get_fields()
    st = int(d["stride"])
    assert np.array_equal(g["rho"][::st, ::st], d["rho_sub"])
    assert np.array_equal(f32(g["u"][::st, ::st]), f32(d["u_sub"])) and np.array_equal(f32(g["v"][::st, ::st]), f32(d["v_sub"]))
    check_against_reference_fixture(d, g["rho"], g["u"], g["v"], 1e-7, 1e-9)
    ua = startup_profile(sim.ny, sim.nx, sim.inlet_rho, sim.lb_viscosity, STEPS)
    assert md(g["u"].mean(axis=0), ua) <= 2e-5
    c = sim._sim.check()
    assert c["n_nonfinite"] == 0 and 0 < c["max_mach"] < 0.3


def test_cpu_backend_is_opt_in_and_refuses_what_it_does_not_do(lbhip):
    from LB_D2Q9 import _native
    from LB_D2Q9.simulation import Simulation
    with pytest.raises(_native.LbError):
        Simulation(32, 16, 1.0, bc="periodic", device=-1, semantics="cython")      # pipe flow only
    with pytest.raises(_native.LbError):
        Simulation(32, 16, 1.0, bc="pipe", device=-1)                              # the OpenCL-path semantics need a GPU
    s = Simulation(32, 16, 1.0, bc="pipe", device=-1, semantics="cython")
    assert s.autotune() == 0                                                       # nothing to choose between
    for call in (s.peer_export, lambda: s.copy_calibration(1), lambda: s.step_boundary()):
        with pytest.raises(_native.LbError):
            call()
    ms = s.timed_run(3)
    assert ms >= 0 and s.steps_per_launch() == 1
    s.close()
