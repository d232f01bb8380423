"""The CPU oracle against (a) fixtures produced by executing the reference's own sources
(oracle/make_golden.py), (b) the reference's analytic Poiseuille known-answer test and (c) the
constants its notebooks print.  No GPU needed.  Fixture comparisons are bit-exact."""
import numpy as np
import pytest

from conftest import golden


def kwargs_of(d):
    kw = dict(zip([str(k) for k in d["kw_names"]], [float(v) for v in d["kw_vals"]]))
    kw["N"] = int(kw["N"])
    return kw


def exact(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- O2: every kernel of D2Q9.cl ------------------------------------------------------------------
def test_o2_each_kernel_bit_exact(oracle):
    O = oracle
    d = golden("o2_kernels_37x19")
    nx, ny = int(d["nx"]), int(d["ny"])

    def fresh():
        s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(d["inlet_rho"]), float(d["outlet_rho"]), mask=d["mask"])
        s.set_f(d["f0"])
        s.fs[...] = d["fs0"].transpose(2, 1, 0)
        return s

    L = O.lib()
    s = fresh()
    L.o2_stream(O._f(s.f), O._f(s.fs), nx, ny, 0, 0)
    assert exact(s.fs.transpose(2, 1, 0), d["after_move_fs"])          # stale entries included
    s = fresh()
    L.o2_bc_pipe(O._f(s.f), np.float32(s.inlet_rho), np.float32(s.outlet_rho), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_f"])
    s = fresh()
    L.o2_bounceback(s.mask.ctypes.data_as(O._ip), O._f(s.f), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bounce_f"])
    s = fresh()
    s.update_hydro()
    assert exact(s.rho.T, d["hydro_rho"]) and exact(s.u.T, d["hydro_u"]) and exact(s.v.T, d["hydro_v"])
    s.update_feq()
    assert exact(s.feq.transpose(2, 1, 0), d["feq"])
    s.collide_particles()
    assert exact(s.f.transpose(2, 1, 0), d["after_collide_f"])
    s.zero_velocity_in_obstacle()
    assert exact(s.u.T, d["zeroed_u"]) and exact(s.v.T, d["zeroed_v"])


def test_o2_each_kernel_bit_exact_on_boundary_obstacles(oracle):
    """The same single calls on o2_edge_mask_61x31, whose solid cells lie on the walls, the inlet, the outlet and the four
    corners: there `move_bcs` and `bounceback_in_obstacle` write the same cell, in that order (opencl_dim.py:510-518)."""
    O = oracle
    d = golden("o2_edge_mask_61x31")
    nx, ny = int(d["nx"]), int(d["ny"])
    m = d["mask"]
    from test_gpu_edge_obstacles import edge_pattern           # the GPU tests' copy of the generator's pattern: kept the same
    assert np.array_equal(edge_pattern(nx, ny), m)
    assert m[0, 0] and m[0, -1] and m[-1, 0] and m[-1, -1]
    assert m[1:-1, 0].any() and m[1:-1, -1].any() and m[0, 1:-1].any() and m[-1, 1:-1].any() and m[1:-1, 1:-1].any()

    def fresh():
        s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(d["inlet_rho"]), float(d["outlet_rho"]), mask=m)
        s.set_f(d["f0"])
        return s

    L = O.lib()
    s = fresh()
    L.o2_bc_pipe(O._f(s.f), np.float32(s.inlet_rho), np.float32(s.outlet_rho), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_f"])
    L.o2_bounceback(s.mask.ctypes.data_as(O._ip), O._f(s.f), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_bounce_f"])
    s = fresh()
    s.move_bcs()                                               # the phase = the two of them
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_bounce_f"])
    assert not exact(d["after_bcs_bounce_f"][m], d["after_bounce_f"][m])      # (the rule is visible under the swap)
    s = fresh()
    L.o2_bounceback(s.mask.ctypes.data_as(O._ip), O._f(s.f), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bounce_f"])
    s = fresh()
    s.update_hydro()
    assert exact(s.rho.T, d["hydro_rho"]) and exact(s.u.T, d["hydro_u"]) and exact(s.v.T, d["hydro_v"])
    s.update_feq()
    assert exact(s.feq.transpose(2, 1, 0), d["feq"])
    s.collide_particles()
    assert exact(s.f.transpose(2, 1, 0), d["after_collide_f"])
    s.zero_velocity_in_obstacle()
    assert exact(s.u.T, d["zeroed_u"]) and exact(s.v.T, d["zeroed_v"])
    assert np.all(s.u.T[m] == 0) and np.all(s.v.T[m] == 0)


@pytest.mark.parametrize("name", ["o2_pipe_N10", "o2_pipe_noise_49x25", "o2_cyl_61x31", "o2_edge_mask_61x31"])
def test_o2_runs_bit_exact(oracle, name):
    O = oracle
    d = golden(name)
    s = O.O2Sim(int(d["nx"]), int(d["ny"]), float(d["omega"]), O.BC_PIPE, float(d["inlet_rho"]),
                float(d["outlet_rho"]), mask=d["mask"] if "mask" in d.files else None)
    s.set_f(d["f0"])
    done = 0
    for n in sorted(int(k[1:-2]) for k in d.files if k.endswith("_u") and k[0] == "s"):
        s.run(n - done)
        done = n
        g = s.get_fields()
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(g[k], d["s%d_%s" % (n, k)]), (name, n, k)


def test_o2_constructor_matches_fixture_and_notebook(oracle):
    """opencl_dim.Pipe_Flow parameter derivation: the N=10 verification case prints
    T=0.387298334621, W=1.16189500386, u_lb=0.1, omega=0.324465802203, inlet rho 1.063
    (docs/opencl_dimensionless_verification.ipynb:94-115); N=50 -> 1.002424, N=200 -> 1.000150375."""
    O = oracle
    d = golden("o2_pipe_N10")
    s = O.O2Sim.pipe_flow(diameter=1.5, rho=10., viscosity=5., pressure_grad=-100., pipe_length=3., N=10)
    p = s.params
    assert (p["nx"], p["ny"]) == (int(d["nx"]), int(d["ny"])) == (21, 11)
    assert p["omega"] == float(d["omega"]) and p["inlet_rho"] == float(d["inlet_rho"])
    assert p["T"] == pytest.approx(0.387298334621, rel=1e-11)
    assert p["W"] == pytest.approx(1.16189500386, rel=1e-11)
    assert p["ulb"] == pytest.approx(0.1) and p["omega"] == pytest.approx(0.324465802203, rel=1e-11)
    assert p["inlet_rho"] == pytest.approx(1.063, rel=1e-12)
    assert exact(s.get_fields()["f"], d["f0"])                 # ramp + feq + f = feq
    for N, rin, glob in ((50, 1.002424, (128, 64)), (200, 1.000150375, (416, 224))):
        q = O.opencl_pipe_parameters(diameter=1.5, rho=10., viscosity=5., pressure_grad=-100., pipe_length=3., N=N)
        assert q["inlet_rho"] == pytest.approx(rin, rel=1e-12)
        assert tuple(-(-v // 32) * 32 for v in (q["nx"], q["ny"])) == glob


# ---- the reference's analytic KAT ---------------------------------------------------------------------
@pytest.mark.parametrize("N,steps,tol", [(10, 999, 0.05), (50, 25000, 0.01)])
def test_o2_poiseuille_profile(oracle, N, steps, tol):
    """docs/opencl_dimensionless_verification.ipynb:279-342, 632-696: after t = 10 the physical
    u(y) at mid-pipe overlays (1/(2 rho nu)) gradP y (y - D); peak 0.5625 m/s."""
    D, rho, nu, gradP = 1.5, 10., 5., -100.
    s = oracle.O2Sim.pipe_flow(diameter=D, rho=rho, viscosity=nu, pressure_grad=gradP, pipe_length=3., N=N)
    p = s.params
    s.run(steps)
    u = s.get_fields()["u"] * (p["delta_x"] / p["delta_t"]) * (p["L"] / p["T"])
    y = np.linspace(0, D, p["ny"])
    theory = (1. / (2 * rho * nu)) * gradP * y * (y - D)
    prof = u[p["nx"] // 2]
    assert theory.max() == pytest.approx(0.5625)
    assert prof[0] == 0. and prof[-1] == 0.                    # no-slip walls, exactly
    assert np.abs(prof - theory).max() < tol * theory.max()


# ---- O1: the Cython path ------------------------------------------------------------------------------
def test_o1_pipe_trace_and_runs_bit_exact(oracle):
    d = golden("o1_pipe_33x17")
    s = oracle.O1Sim.pipe_flow(perturb=d["perturb"], **kwargs_of(d))
    assert (s.nx, s.ny) == (int(d["nx"]), int(d["ny"]))
    assert s.omega == float(d["omega"]) and s.inlet_rho == float(d["inlet_rho"])
    assert exact(s.rho, d["rho0"]) and exact(s.f, d["f0"])
    s.run(2)
    for k in ("f", "feq", "rho", "u", "v"):
        assert exact(s.get_fields()[k], d["pre_" + k]), k
    s.move_bcs();          assert exact(s.f, d["t_bcs_f"])
    s.move();              assert exact(s.f, d["t_move_f"])
    s.update_hydro()
    assert exact(s.rho, d["t_hydro_rho"]) and exact(s.u, d["t_hydro_u"]) and exact(s.v, d["t_hydro_v"])
    s.update_feq();        assert exact(s.feq, d["t_feq"])
    s.collide_particles(); assert exact(s.f, d["t_collide_f"])
    done = 3
    for n in (50, 500):
        s.run(n - done)
        done = n
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(s.get_fields()[k], d["s%d_%s" % (n, k)]), (n, k)


def test_o1_cylinder_bit_exact(oracle):
    d = golden("o1_cyl_61x41")
    s = oracle.O1Sim.pipe_flow(cylinder_center=list(d["cylinder_center"]), cylinder_radius=float(d["cylinder_radius"]),
                               perturb=d["perturb"], **kwargs_of(d))
    assert exact(s.mask.astype(bool), d["mask"])               # disc restatement == the mask the reference built
    assert s.omega == float(d["omega"]) and s.inlet_rho == float(d["inlet_rho"])
    done = 0
    for n in (1, 50, 300):
        s.run(n - done)
        done = n
        g = s.get_fields()
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(g[k], d["s%d_%s" % (n, k)]), (n, k)
        assert np.all(g["u"][d["mask"]] == 0)


@pytest.mark.parametrize("name,edge", [("o1_edge_cyl_61x41", "south"), ("o1_edge_cyl_inlet_61x41", "inlet")])
def test_o1_cylinder_on_the_boundary_bit_exact(oracle, name, edge):
    """The cylinder of o1_cyl_61x41 moved until five of its cells lie on the south wall row / on the inlet column."""
    d = golden(name)
    s = oracle.O1Sim.pipe_flow(cylinder_center=list(d["cylinder_center"]), cylinder_radius=float(d["cylinder_radius"]),
                               perturb=d["perturb"], **kwargs_of(d))
    assert exact(s.mask.astype(bool), d["mask"])
    assert int((d["mask"][:, 0] if edge == "south" else d["mask"][0, :]).sum()) == 5
    assert s.omega == float(d["omega"]) and s.inlet_rho == float(d["inlet_rho"])
    assert exact(s.f, d["f0"])
    done = 0
    for n in (1, 50, 300):
        s.run(n - done)
        done = n
        g = s.get_fields()
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(g[k], d["s%d_%s" % (n, k)]), (n, k)
        assert np.all(g["u"][d["mask"]] == 0) and np.all(g["v"][d["mask"]] == 0)


def test_o1_numpy1_mode_stays_within_one_ulp_per_step(oracle):
    """numpy2=0 restates what the authors' NumPy 1.x computed (float32 collide); it is unpinned
    but must track the pinned numpy2=1 mode closely."""
    d = golden("o1_pipe_33x17")
    a = oracle.O1Sim.pipe_flow(perturb=d["perturb"], numpy2=True, **kwargs_of(d))
    b = oracle.O1Sim.pipe_flow(perturb=d["perturb"], numpy2=False, **kwargs_of(d))
    a.run(100); b.run(100)
    assert np.abs(a.rho - b.rho).max() < 5e-6 and np.abs(a.u - b.u).max() < 5e-6


def test_cython_constructor_constants(oracle):
    """Derived constants of the Cython-style classes: values printed by the notebooks
    (docs/python_cython_opencl_comparison.ipynb cell 10-13, docs/vortex_sheet_movie.ipynb:98-154,
    docs/cs205_movie.ipynb:98-154) and the same quantities read back from the imported reference."""
    O = oracle
    p = O.cython_pipe_parameters(diameter=1., rho=1., viscosity=1., pressure_grad=-10., pipe_length=3., N=125,
                                 cylinder_radius=.1)
    assert p["L"] == pytest.approx(0.1) and p["T"] == pytest.approx(0.08) and p["Re"] == pytest.approx(1.5625)
    assert p["omega"] == pytest.approx(0.413223140496, rel=1e-11)
    assert (p["nx"], p["ny"]) == (3751, 1251) and p["inlet_rho"] == pytest.approx(1.00368738304, rel=1e-11)
    t = golden("o1_constants")["table"]
    for N, r, L, T, Re, omega, rin, nx, ny in t:
        q = O.cython_pipe_parameters(diameter=1., rho=1., viscosity=1., pressure_grad=-100., pipe_length=3.,
                                     N=int(N), cylinder_radius=r)
        assert (q["L"], q["T"], q["Re"], q["omega"], q["inlet_rho"], q["nx"], q["ny"]) == (L, T, Re, omega, rin, nx, ny)
    assert t[0][4] == pytest.approx(156.25) and t[0][5] == pytest.approx(1.92604006163, rel=1e-11)
    assert t[0][6] == pytest.approx(1.0092209152, rel=1e-10) and t[1][6] == pytest.approx(1.009228288, rel=1e-10)


# ---- cross-semantics sanity (the reference authors' own finding) ---------------------------------------------
def test_o1_and_o2_agree_in_the_interior_on_the_first_step(oracle):
    """testing/Bryan/opencl_check_03.ipynb:593,778: the two implementations agree to 1e-6 away from
    walls and corners.  Identical rest state on the density ramp, one step."""
    O = oracle
    nx, ny, omega, rin = 48, 24, 1.0, 1.004
    ramp = O.density_ramp(nx, ny, rin, 1.)
    o2 = O.O2Sim(nx, ny, omega, O.BC_PIPE, rin, 1.)
    o2.set_macro(ramp, 0 * ramp, 0 * ramp); o2.update_feq(); o2.init_pop()
    o1 = O.O1Sim(nx, ny, omega, rin, 1.)
    o1.rho[...] = ramp; o1.update_feq(); o1.init_pop()
    o1.run(1); o2.run(1)
    g = o2.get_fields()
    inner = (slice(3, -3), slice(3, -3))
    assert np.abs(g["rho"][inner] - o1.rho[inner]).max() <= 1e-6
    assert np.abs(g["u"][inner] - o1.u[inner]).max() <= 1e-6


def test_o1_and_o2_agree_outside_the_walls_domain_of_dependence_for_ten_steps(oracle):
    """The same comparison over ten steps.  The two paths use different wall / inlet rules, and
    what a wall does travels one cell per step, so after n steps the 1e-6 agreement is required of the cells
    more than n + 2 cells away from every wall (the reference authors' 3-cell margin at n = 1); with the fixed
    3-cell margin it is lost after four steps (measured: 8e-7 in rho at step 4, 7e-6 at step 10)."""
    O = oracle
    nx, ny, omega, rin = 96, 64, 1.0, 1.004
    ramp = O.density_ramp(nx, ny, rin, 1.)
    o2 = O.O2Sim(nx, ny, omega, O.BC_PIPE, rin, 1.)
    o2.set_macro(ramp, 0 * ramp, 0 * ramp); o2.update_feq(); o2.init_pop()
    o1 = O.O1Sim(nx, ny, omega, rin, 1.)
    o1.rho[...] = ramp; o1.update_feq(); o1.init_pop()
    for n in range(1, 11):
        o1.run(1); o2.run(1)
        g = o2.get_fields()
        m = n + 2
        inner = (slice(m, -m), slice(m, -m))
        assert np.abs(g["rho"][inner] - o1.rho[inner]).max() <= 1e-6, n
        assert np.abs(g["u"][inner] - o1.u[inner]).max() <= 1e-6 and np.abs(g["v"][inner] - o1.v[inner]).max() <= 1e-6, n
        f1 = o1.f.transpose(1, 2, 0)
        assert np.abs(g["f"][inner] - f1[inner]).max() <= 1e-6, n


def test_o2_velocity_inlet_kernels_bit_exact(oracle):
    """D2Q9.cl:263-374 (`move_bcs_PeriodicBC_VelocityInlet`, `update_hydro_PeriodicBC_VelocityInlet`), executed
    through the same C shim as the other kernels, driven as OLD/opencl.py:281-327 drives them."""
    O = oracle
    d = golden("o2_velocity_inlet_45x23")
    nx, ny, uw = int(d["nx"]), int(d["ny"]), float(d["u_w"])
    s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_VELOCITY_INLET, u_w=uw)
    s.set_f(d["f0"])
    O.lib().o2_bc_velocity_inlet(O._f(s.f), np.float32(uw), np.float32(uw), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_f"])
    s.set_f(d["f0"])
    s.set_macro(np.ones((nx, ny)), np.full((nx, ny), uw), np.zeros((nx, ny)))
    s.update_hydro()
    assert exact(s.rho.T, d["hydro_rho"]) and exact(s.u.T, d["hydro_u"]) and exact(s.v.T, d["hydro_v"])
    s.set_macro(np.ones((nx, ny)), np.full((nx, ny), uw), np.zeros((nx, ny)))
    done = 0
    for n in (1, 20, 200):
        s.run(n - done)
        done = n
        g = s.get_fields()
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(g[k], d["s%d_%s" % (n, k)]), (n, k)


def test_o2_d2q9i_fork_bit_exact_and_unstable(oracle):
    """LB_D2Q9/D2Q9i.cl (SURVEY: experimental fork, used by no notebook).  The oracle restates its three
    differing routines bit-exactly - and the executed reference itself diverges: |u| grows ~10x in ten
    steps from a 2e-4 density drop and is NaN by step 60.  That is why the engine does not offer it."""
    O = oracle
    d = golden("o2_d2q9i_53x27")
    nx, ny = int(d["nx"]), int(d["ny"])

    def fresh():
        s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(d["inlet_rho"]), float(d["outlet_rho"]),
                    mask=d["mask"], d2q9i=True)
        s.set_f(d["f0"])
        return s

    s = fresh()
    O.lib().o2i_bc_pipe(O._f(s.f), np.float32(s.inlet_rho), np.float32(s.outlet_rho), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_f"])
    s = fresh()
    O.lib().o2i_moments(O._f(s.f), O._f(s.rho), O._f(s.u), O._f(s.v), nx, ny)
    assert exact(s.rho.T, d["hydro_rho"]) and exact(s.u.T, d["hydro_u"]) and exact(s.v.T, d["hydro_v"])
    s.update_feq()
    assert exact(s.feq.transpose(2, 1, 0), d["feq1"])
    s = fresh()
    s.run(1)
    for k in ("f", "feq", "rho", "u", "v"):
        assert exact(s.get_fields()[k], d["s1_" + k]), k
    s.run(9)
    for k in ("f", "rho", "u", "v"):
        assert exact(s.get_fields()[k], d["s10_" + k]), k
    assert np.abs(d["s10_u"]).max() > 10 * np.abs(d["s1_u"]).max()        # already running away
    assert np.isnan(d["s60_u"]).any()                                     # the reference execution blew up


# ---- outlet_rho, rho0 and the fluid's density off 1 ------------------------------------------------------------------------
# Every fixture above has outlet_rho = 1.0 and the oracle's other users pass rho0 = 1.0: there `x / rout` and the products with
# rout lose a rounding step, and a rule reading the wrong one of its two densities computes the same.
def test_o2_boundary_densities_off_one_bit_exact(oracle):
    """o2_offone_37x19 (D2Q9.cl executed at (0.9337, 0.93) and (1.0743, 1.07), the fluid at the outlet's density): `move_bcs`,
    `update_hydro`, then 1, 10 and 50 steps."""
    O = oracle
    d = golden("o2_offone_37x19")
    nx, ny = int(d["nx"]), int(d["ny"])
    assert [tuple(p) for p in zip(d["inlet_rho"], d["outlet_rho"])] == [(0.9337, 0.93), (1.0743, 1.07)]
    for i, (rin, rout) in enumerate(zip(d["inlet_rho"], d["outlet_rho"])):
        p = "p%d_" % i

        def fresh():
            s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(rin), float(rout), mask=d["mask"])
            s.set_f(d[p + "f0"])
            return s

        assert abs(float(d[p + "f0"].sum(axis=2, dtype=np.float64).mean()) / rout - 1) < 2e-3      # (the fluid IS off 1)
        s = fresh()
        s.fs[...] = d["fs0"].transpose(2, 1, 0)
        O.lib().o2_bc_pipe(O._f(s.f), np.float32(rin), np.float32(rout), nx, ny)
        assert exact(s.f.transpose(2, 1, 0), d[p + "after_bcs_f"])
        s = fresh()
        s.update_hydro()
        assert exact(s.rho.T, d[p + "hydro_rho"]) and exact(s.u.T, d[p + "hydro_u"]) and exact(s.v.T, d[p + "hydro_v"])
        s = fresh()
        done = 0
        for n in (1, 10, 50):
            s.run(n - done)
            done = n
            g = s.get_fields()
            for k in ("f", "feq", "rho", "u", "v"):
                assert exact(g[k], d["%ss%d_%s" % (p, n, k)]), (i, n, k)
        # the parameter is visible: the same run with outlet_rho = 1 leaves the fixture on the outlet column at once
        t = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(rin), 1., mask=d["mask"])
        t.set_f(d[p + "f0"])
        t.run(1)
        diff = np.abs(t.get_fields()["f"] - d[p + "s1_f"]).max(axis=2)
        assert diff[-1].min() > 1e-2 and diff[:-1].max() == 0


def test_o2_d2q9i_boundary_densities_off_one_bit_exact(oracle):
    """o2_d2q9i_offone_37x19: D2Q9i.cl executed at (1.0002, 0.9998), fluid at 1, inside the fork's stable window."""
    O = oracle
    d = golden("o2_d2q9i_offone_37x19")
    nx, ny = int(d["nx"]), int(d["ny"])
    assert (float(d["inlet_rho"]), float(d["outlet_rho"])) == (1.0002, 0.9998)

    def fresh():
        s = O.O2Sim(nx, ny, float(d["omega"]), O.BC_PIPE, float(d["inlet_rho"]), float(d["outlet_rho"]), mask=d["mask"], d2q9i=True)
        s.set_f(d["f0"])
        return s

    s = fresh()
    O.lib().o2i_bc_pipe(O._f(s.f), np.float32(s.inlet_rho), np.float32(s.outlet_rho), nx, ny)
    assert exact(s.f.transpose(2, 1, 0), d["after_bcs_f"])
    s = fresh()
    done = 0
    for n in (1, 8):
        s.run(n - done)
        done = n
        g = s.get_fields()
        for k in ("f", "feq", "rho", "u", "v"):
            assert exact(g[k], d["s%d_%s" % (n, k)]), (n, k)
    assert np.abs(d["s8_u"]).max() < 0.02


def column_sums(f_xyk):
    """sum_k f in float64: (nx, ny)"""
    return np.asarray(f_xyk, np.float64).sum(axis=2)


def assert_imposed_density(f_xyk, mask, bc, rho_w, rho_e, rho_corner=None):
    """What the boundary rules were derived from, on the populations one `move_bcs` call leaves: a pressure inlet / outlet
    closes its three unknown links so that sum_k f = the imposed density (uu = +-(1 - S / rho) with S the known links counted
    as the column sees them, and the three new links add rho uu to them), a corner's two free links are set to half of what
    the density lacks.  Each rule ends in three or four float32 roundings: 4 * 2^-24 rho.  Non-solid cells (the swap that
    follows the rule permutes a solid cell's links; it is left out all the same).  Pipe: inlet and outlet column, corners
    included; cavity: the four corners (rho_corner)."""
    S = column_sums(f_xyk)
    fluid = ~np.asarray(mask, bool) if mask is not None else np.ones(S.shape, bool)
    checks = []
    if bc == "pipe":
        checks += [("inlet", S[0][fluid[0]], rho_w), ("outlet", S[-1][fluid[-1]], rho_e)]
    else:
        corners = [(0, 0), (0, -1), (-1, 0), (-1, -1)]
        checks += [("corners", np.array([S[c] for c in corners if fluid[c]]), rho_corner)]
    worst = 0.
    for what, sums, rho in checks:
        if sums.size:
            err = float(np.abs(sums - float(np.float32(rho))).max())
            worst = max(worst, err / (4 * 2.0 ** -24 * rho))
            assert err <= 4 * 2.0 ** -24 * rho, (bc, what, err, 4 * 2.0 ** -24 * rho)
    return worst


@pytest.mark.parametrize("nx,ny", [(37, 19), (5, 7), (3, 3)])
def test_boundary_rules_impose_their_density(oracle, nx, ny):
    """The analytic property on the oracle's own output, in float64.  For the cavity closure the oracle is otherwise its own
    definition: this is its check."""
    O = oracle
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    rng = np.random.default_rng(nx * 100 + ny)
    mask = rng.random((nx, ny)) < 0.05
    mask[0, ny // 2] = mask[-1, ny // 2] = True                      # (one solid cell on the inlet and on the outlet column)
    for bc, kw, fluid in ([(O.BC_PIPE, dict(inlet_rho=a, outlet_rho=b), b) for a, b in ((0.9337, 0.93), (1.0743, 1.07), (1.004, 1.0))] +
                          [(O.BC_CAVITY, dict(lid_u=0.06, rho0=r), r) for r in (0.93, 1.07, 1.0)]):
        for m in (None, mask):
            f0 = (fluid * w[None, None, :] * (1 + 0.02 * rng.standard_normal((nx, ny, 9)))).astype(np.float32)
            s = O.O2Sim(nx, ny, 1.6, bc, mask=m, **kw)
            s.set_f(f0)
            s.move_bcs()
            f = s.get_fields()["f"]
            if bc == O.BC_PIPE:
                assert_imposed_density(f, m, "pipe", kw["inlet_rho"], kw["outlet_rho"])
            else:
                assert_imposed_density(f, m, "cavity", None, None, kw["rho0"])
    for rin, rout in ((1.0002, 0.9998), (1.0004, 1.0002)):           # the fork's own inlet and outlet
        f0 = (w[None, None, :] * (1 + 0.001 * rng.standard_normal((nx, ny, 9)))).astype(np.float32)
        s = O.O2Sim(nx, ny, 1.0, O.BC_PIPE, rin, rout, mask=mask, d2q9i=True)
        s.set_f(f0)
        s.move_bcs()
        assert_imposed_density(s.get_fields()["f"], mask, "pipe", rin, rout)


def test_periodic_family_taylor_green_decay_rate(oracle):
    """The periodic family is build-defined (the reference's `dimensionless` package has no periodic streaming), so the
    oracle's [BD] routine is anchored to physics instead: a Taylor-Green vortex must decay with the lattice viscosity
    nu = (1/omega - 1/2)/3, energy ~ exp(-4 nu k^2 t) (same test on the GPU: tests/test_gpu_physics.py)."""
    n, U, omega = 64, 0.02, 1.2
    nu, k = (1. / omega - 0.5) / 3., 2 * np.pi / n
    x = np.arange(n)[:, None] * np.ones((1, n))
    y = np.ones((n, 1)) * np.arange(n)[None, :]
    u0 = U * np.cos(k * x) * np.sin(k * y)
    v0 = -U * np.sin(k * x) * np.cos(k * y)
    rho0 = 1. - 0.75 * U * U * (np.cos(2 * k * x) + np.cos(2 * k * y))
    s = oracle.O2Sim(n, n, omega, oracle.BC_PERIODIC)
    s.set_macro(rho0, u0, v0)
    s.update_feq(); s.init_pop()
    e, t = [], []
    for steps in (50, 100, 200, 400):
        s.run(steps - (t[-1] if t else 0))
        t.append(steps)
        g = s.get_fields()
        e.append(float((g["u"].astype(np.float64) ** 2 + g["v"].astype(np.float64) ** 2).mean()))
    rate = -np.polyfit(np.array(t, float), np.log(np.array(e)), 1)[0]
    assert rate == pytest.approx(4 * nu * k * k, rel=0.02)


def test_periodic_streaming_is_the_forks_move_periodic(oracle):
    """The oracle's periodic streaming ([BD] in d2q9_oracle.c: no counterpart in LB_D2Q9/dimensionless) against the one
    periodic kernel the reference has, executed: porous_media/single_component.cl:338-375 `move_periodic`
    (fixture o2_move_periodic, oracle/make_golden.py gen_move_periodic; integer-valued entries, exact).  Also pins the
    `np.roll` restatement the GPU test uses at sizes the fixture does not hold."""
    d = golden("o2_move_periodic")
    cx = [0, 1, 0, -1, 0, 1, -1, -1, 1]
    cy = [0, 0, 1, 0, -1, 1, 1, -1, -1]
    for tag in "abc":
        f, want = d["f_" + tag], d["streamed_" + tag]               # (nx, ny, P, 9)
        nx, ny, P, J = f.shape
        assert J == 9 and sorted(want.ravel()) == sorted(f.ravel())
        rolled = np.empty_like(f)
        for j in range(9):
            rolled[:, :, :, j] = np.roll(np.roll(f[:, :, :, j], cx[j], axis=0), cy[j], axis=1)
        assert np.array_equal(rolled, want)
        for i in range(P):
            o = oracle.O2Sim(nx, ny, 1.0, oracle.BC_PERIODIC)
            o.set_f(f[:, :, i, :].astype(np.float32))
            o.move()
            assert np.array_equal(o.get_fields()["f"], want[:, :, i, :].astype(np.float32)), (tag, i)


def test_o2_openmp_build_gives_the_serial_build_its_bits(oracle):
    """The -fopenmp build of the OpenCL-path oracle (used to hold the 8192^2 GPU run to the oracle in seconds,
    tests/test_gpu_fullsize.py) runs the same per-cell arithmetic over independent loops: bitwise equal to the serial
    build -- which the fixtures pin -- in every family, with an obstacle mask."""
    rng = np.random.default_rng(5)
    nx, ny = 61, 47
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    f0 = (w[None, None, :] * (1 + 0.02 * rng.standard_normal((nx, ny, 9)))).astype(np.float32)
    mask = rng.random((nx, ny)) < 0.05
    mask[0, :] = mask[-1, :] = False
    mask[:, 0] = mask[:, -1] = False
    for bc, kw in ((oracle.BC_PERIODIC, {}), (oracle.BC_PIPE, dict(inlet_rho=1.01, outlet_rho=1.0)),
                   (oracle.BC_CAVITY, dict(lid_u=0.07, rho0=1.0))):
        a = oracle.O2Sim(nx, ny, 1.7, bc, mask=mask, **kw)
        b = oracle.O2Sim(nx, ny, 1.7, bc, mask=mask, **kw)
        a.set_f(f0); b.set_f(f0)
        a.run(12); b.run(12, openmp=True)
        for k in ("f", "rho", "u", "v", "feq"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (bc, k)
