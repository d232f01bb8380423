"""Coupled scalar lattices: several concentrations on one grid that share an imposed velocity field and compete for room.

The reference's ``advecting_range_expansion`` fork (``D2Q9_multifield_fisher.cl``) keeps ``num_populations`` fields in
arrays shaped ``(nx, ny, num_populations[, 9])`` (Fortran order) and loops over them in every work-item of five launches
per step.  Here every field is one engine lattice (``Simulation(semantics='multifield')``, its own ``omega`` and ``G``) and
``run(n)`` advances all of them with ONE fused launch per time step (``lb_run_coupled``): per cell, field i relaxes
towards ``w_k rho_i (1 + 3 c_k.u)`` and grows by ``w_k G_i rho_i (1 - sum_j rho_j)``.  ``bc='box'`` is the fork's closed
box (on-node bounce-back on all four walls), ``bc='periodic'`` wraps.  The phase methods run the fork's kernels one by
one.  The velocity the fused step reads is the first member's; ``set_fields`` / ``set_velocity_from`` write every member.

``Advected_Scalars`` at the end pairs a live flow with the scalar lattices it carries (``lb_run_advected``).
"""
import ctypes as ct

import numpy as np

from . import _native
from ._native import check
from .simulation import NUM_JUMPERS, Simulation


class _Lattice_Set(object):
    """What the sets share: the members (one ``Simulation`` each) and the ctypes array of their handles, state as arrays shaped
    ``(nx, ny, num_populations[, 9])``, the phases every member makes on its own, ``run`` / ``step`` through the class's entry
    point, ``get_fields`` by the class's key lists, and the ``m<i>_`` entries of a checkpoint."""
    _RUN = None             # the library's run entry point for this kind of set
    _STACKED = ()           # get_fields keys that every member has: stacked along axis 2
    _SHARED = ()            # ... that the members share: read from the first
    _OWN = ()               # ... that the set itself keeps: _read_own

    def _adopt(self, nx, ny, members):
        self.nx, self.ny, self.num_populations, self.num_jumpers = int(nx), int(ny), len(members), NUM_JUMPERS
        self.members = members
        self._lib = _native.lib()
        self._handles = (ct.c_void_p * len(members))(*[m._h for m in members])

    def _call(self, entry, *args):
        """One of the library's calls on the whole set."""
        check(getattr(self._lib, entry)(self._handles, self.num_populations, *args))

    def close(self):
        for m in self.members:
            m.close()

    def sync(self):
        for m in self.members:
            m.sync()

    def _per_field(self, a, tail=()):
        a = np.asarray(a)
        if a.shape != (self.nx, self.ny, self.num_populations) + tail:
            raise ValueError("expected shape %r" % ((self.nx, self.ny, self.num_populations) + tail,))
        return a

    # -- state: arrays shaped like the fork's (nx, ny, num_populations[, 9]), Fortran order ------------------------------
    def set_f(self, f):
        f = self._per_field(f, (self.num_jumpers,))
        for i, m in enumerate(self.members):
            m.set_f(f[:, :, i, :])

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb on every member; perturb None or (nx, ny, num_populations, 9)."""
        for i, m in enumerate(self.members):
            m.init_pop(None if perturb is None else np.asarray(perturb)[:, :, i, :])

    def _get_fields(self, which):
        out = {}
        stacked = tuple(k for k in which if k in self._STACKED)
        if stacked:
            per = [m.get_fields(stacked) for m in self.members]
            for k in stacked:
                out[k] = np.asfortranarray(np.stack([g[k] for g in per], axis=2))
        shared = tuple(k for k in which if k in self._SHARED)
        if shared:
            out.update(self.members[0].get_fields(shared))
        own = [k for k in which if k in self._OWN]
        if own:
            self._read_own(own, out)
        return out

    # -- the phases every member makes on its own, un-fused ----------------------------------------------------------------
    def move(self):
        for m in self.members:
            m.move()

    def move_bcs(self):
        for m in self.members:
            m.move_bcs()

    def update_hydro(self):
        for m in self.members:
            m.update_hydro()

    def update_feq(self):
        for m in self.members:
            m.update_feq()

    # -- the hot path ---------------------------------------------------------------------------------------------------
    def run(self, num_iterations, wait=True):
        """num_iterations fused time steps of all members, one launch per step."""
        self._call(self._RUN, int(num_iterations))
        if wait:
            self.sync()

    def step(self):
        self.run(1)

    # -- checkpoints: every member's arrays under 'm<i>_' ------------------------------------------------------------------
    def _member_entries(self):
        return {"m%d_%s" % (i, k): a for i, m in enumerate(self.members) for k, a in m.checkpoint_arrays().items()}

    @staticmethod
    def _load_entries(path):
        """(the set's own entries, [every member's, without the prefix]) of a checkpoint file"""
        with np.load(Simulation._ckpt_path(path)) as d:
            per = []
            while "m%d_version" % len(per) in d.files:
                prefix = "m%d_" % len(per)
                per.append({k[len(prefix):]: d[k] for k in d.files if k.startswith(prefix)})
            return {k: d[k] for k in d.files if not any(k.startswith("m%d_" % i) for i in range(len(per)))}, per


class _Shared_Velocity(object):
    """Scalar lattices advected by one velocity field."""

    def set_fields(self, rho, u, v):
        """rho: (nx, ny, num_populations); u, v: (nx, ny), written to every member."""
        rho = self._per_field(rho)
        for i, m in enumerate(self.members):
            m.set_fields(rho[:, :, i], u, v)

    def check(self):
        """Per member: Simulation.check() (non-finite cells, max Mach number of the imposed field, sum of rho)."""
        return [m.check() for m in self.members]


class _Fused_Set(_Lattice_Set):
    """A set whose step is one launch or, under ``set_variant(0)``, two; it has a checkpoint file of its own."""

    def set_variant(self, variant):
        for m in self.members:
            m.set_variant(variant)

    def hot_kernel(self):
        return self.members[0].hot_kernel()

    def save_checkpoint(self, path):
        np.savez(Simulation._ckpt_path(path), **dict(self._own_entries(), **self._member_entries()))


class Coupled_Scalars(_Shared_Velocity, _Lattice_Set):
    MAX_POPULATIONS = 4
    _RUN, _STACKED, _SHARED = "lb_run_coupled", ("f", "feq", "rho"), ("u", "v")

    def __init__(self, nx, ny, omegas, Gs, bc="box", device=0, planar=None):
        omegas, Gs = [float(o) for o in np.atleast_1d(omegas)], [float(g) for g in np.atleast_1d(Gs)]
        if not 1 <= len(omegas) <= self.MAX_POPULATIONS or len(Gs) != len(omegas):
            raise ValueError("1..%d fields, one omega and one G each" % self.MAX_POPULATIONS)
        if bc not in ("box", "periodic"):
            raise ValueError("bc must be 'box' or 'periodic'")
        self.omegas, self.Gs, self.bc = omegas, Gs, bc
        self._adopt(nx, ny, [Simulation(nx, ny, om, bc=bc, semantics="multifield", device=device, planar=planar) for om in omegas])
        for m, g in zip(self.members, Gs):
            m.set_reaction(g)

    def set_velocity_from(self, flow):
        """u, v of a flow Simulation of the same grid become every member's imposed velocity, device to device."""
        for m in self.members:
            m.set_velocity_from(flow)

    def get_fields(self, which=("f", "feq", "u", "v", "rho")):
        """f, feq: (nx, ny, num_populations, 9); rho: (nx, ny, num_populations); u, v: (nx, ny) (the first member's)."""
        return self._get_fields(which)

    def get_corner_state(self):
        """(num_populations, 8): every member's never-written corner links (bc='box'; include/lb_hip.h)."""
        return np.stack([m.get_corner_state() for m in self.members])

    def set_corner_state(self, values):
        values = np.asarray(values, np.float32)
        if values.shape != (self.num_populations, 8):
            raise ValueError("corner state = (num_populations, 8) floats")
        for m, v in zip(self.members, values):
            m.set_corner_state(v)

    def collide_particles(self):
        self._call("lb_collide_coupled")
        self.sync()


class Shan_Chen_Fluids(_Fused_Set):
    """A set of 1..3 fluids on one grid (``Simulation(semantics='multifluid')``, its own ``omega`` each) that relax towards
    their common barycentric velocity and act on each other through pseudopotential forces and reactions: the reference's
    ``multicomponent_multiphase/multi.py``.  ``run(n)`` advances all of them with one launch per time step and no host
    wait (``lb_run_fluids``: the densities of a workgroup's rows and their halo in LDS; ``set_variant(0)``: two launches, the
    densities through memory; the same bits); the phase methods run the reference's stages one by one and equal it bitwise.  Arrays are
    shaped like the reference's, ``(nx, ny, num_populations[, 9])`` in Fortran order; ``u_bary``, ``v_bary`` are ``(nx, ny)``.

    ``interactions``: rows ``(fluid_1, fluid_2, G_int, potential, parameter)`` with potential ``'linear'``, ``'shan_chen'``
    (parameter rho_0) or ``'pow'`` (parameter alpha); the stencil's boundary rule is the set's family.  ``reactions``: rows
    ``('eat', eater, eatee, rate, cutoff)`` or ``('grow', fluid, min, max, rate)``, applied in order."""
    MAX_POPULATIONS = _native.MC_MAX
    POTENTIALS = {"linear": _native.LB_PSI_LINEAR, "shan_chen": _native.LB_PSI_SHAN_CHEN, "pow": _native.LB_PSI_POW}
    _RUN, _STACKED, _SHARED = "lb_run_fluids", ("f", "feq", "rho", "u", "v", "Gx", "Gy"), ("u_bary", "v_bary")

    def __init__(self, nx, ny, omegas, bc="periodic", device=0, planar=None):
        omegas = [float(o) for o in np.atleast_1d(omegas)]
        if not 1 <= len(omegas) <= self.MAX_POPULATIONS:
            raise NotImplementedError("1..%d fluids are built (more than %d fluids are not)" % (self.MAX_POPULATIONS, self.MAX_POPULATIONS))
        if bc not in ("periodic", "zero_gradient"):
            raise ValueError("bc must be 'periodic' or 'zero_gradient'")
        self.omegas, self.bc = omegas, bc
        self._adopt(nx, ny, [Simulation(nx, ny, om, bc=bc, semantics="multifluid", device=device, planar=planar) for om in omegas])
        self.interactions, self.reactions = [], []

    @classmethod
    def of(cls, members):
        """The set made of existing ``Simulation(semantics='multifluid')`` objects, in this order (they stay their owners')."""
        members = list(members)
        if not 1 <= len(members) <= cls.MAX_POPULATIONS:
            raise NotImplementedError("1..%d fluids are built (more than %d fluids are not)" % (cls.MAX_POPULATIONS, cls.MAX_POPULATIONS))
        if len({m.bc_mode for m in members}) != 1:
            raise NotImplementedError("fluids of different families in one set are not built")
        self = cls.__new__(cls)
        self.omegas = [m.omega for m in members]
        self.bc = "periodic" if members[0].bc_mode == _native.LB_BC_PERIODIC else "zero_gradient"
        self._adopt(members[0].nx, members[0].ny, members)
        self.interactions, self.reactions = [], []
        return self

    # -- the tables ---------------------------------------------------------------------------------------------------------
    def set_interactions(self, table):
        rows = []
        for f1, f2, G_int, potential, parameter in table:
            if potential not in self.POTENTIALS:
                raise NotImplementedError("potential %r is not built (linear, shan_chen and pow are; vdw is not)" % (potential,))
            rows.append((int(f1), int(f2), self.POTENTIALS[potential], 0 if self.bc == "periodic" else 1, G_int, parameter))
        self.members[0]._set_tables(self._handles, self.num_populations, rows, None)
        self.interactions = [tuple(r) for r in table]

    def set_reactions(self, table):
        rows = []
        for r in table:
            if r[0] == "eat":
                rows.append((_native.LB_REACT_EAT, int(r[1]), int(r[2]), r[3], r[4], 0.))
            elif r[0] == "grow":
                rows.append((_native.LB_REACT_GROW, int(r[1]), 0, r[2], r[3], r[4]))
            else:
                raise ValueError("a reaction is ('eat', eater, eatee, rate, cutoff) or ('grow', fluid, min, max, rate)")
        self.members[0]._set_tables(self._handles, self.num_populations, None, rows)
        self.reactions = [tuple(r) for r in table]

    # -- state --------------------------------------------------------------------------------------------------------------
    def set_fields(self, rho, u=None, v=None):
        """rho, and optionally the stored component velocities u, v: (nx, ny, num_populations) each."""
        rho = self._per_field(rho)
        zero = np.zeros((self.nx, self.ny), np.float32)
        for i, m in enumerate(self.members):
            m.set_fields(rho[:, :, i], zero if u is None else self._per_field(u)[:, :, i], zero if v is None else self._per_field(v)[:, :, i])

    def set_bary_velocity(self, u_bary, v_bary):
        for m in self.members:
            m.set_bary_velocity(u_bary, v_bary)

    def set_body_force(self, fluid, gx, gy):
        self.members[int(fluid)].set_body_force(gx, gy)

    def set_force_field(self, fluid, gx, gy):
        self.members[int(fluid)].set_force_field(gx, gy)

    def get_fields(self, which=("f", "feq", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary")):
        return self._get_fields(which)

    # -- the reference's stages that involve the whole set, un-fused -------------------------------------------------------
    def update_forces(self):
        self._call("lb_update_forces_fluids")
        self.sync()

    def update_bary_velocity(self):
        self._call("lb_update_bary_fluids")
        self.sync()

    def collide_particles(self):
        for m in self.members:
            m.collide_particles()

    def react(self):
        self._call("lb_react_fluids")
        self.sync()

    def step_phases(self):
        """One time step as the reference's run loop makes it, stage by stage (each call waits)."""
        self.move()
        self.move_bcs()
        self.update_hydro()
        self.update_forces()
        self.update_bary_velocity()
        self.update_feq()
        self.collide_particles()
        self.react()

    # -- checkpoints: every member's arrays under 'm<i>_', the tables with the first ----------------------------------------
    def _own_entries(self):
        return {"num_populations": self.num_populations}

    @classmethod
    def from_checkpoint(cls, path, device=0):
        _, per = cls._load_entries(path)
        bc = {_native.LB_BC_PERIODIC: "periodic", _native.LB_BC_ZERO_GRADIENT: "zero_gradient"}[int(per[0]["bc_mode"])]
        out = cls(int(per[0]["nx"]), int(per[0]["ny"]), [float(p["omega"]) for p in per], bc=bc, device=device)
        for m, p in zip(out.members, per):
            m.restore_arrays(p)
        names = {v: k for k, v in cls.POTENTIALS.items()}
        out.set_interactions([(int(r[0]), int(r[1]), r[4], names[int(r[2])], r[5]) for r in per[0]["interactions"]])
        out.set_reactions([("eat", int(r[1]), int(r[2]), r[3], r[4]) if int(r[0]) == _native.LB_REACT_EAT else ("grow", int(r[1]), r[3], r[4], r[5])
                           for r in per[0]["reactions"]])
        return out


class Surfactant_Colony(_Shared_Velocity, _Fused_Set):
    """A growing population and the surfactant it secretes, two scalar lattices in one periodic box
    (``Simulation(semantics='rocket')``, ``omega`` and ``omega_c``): the reference's ``rocket_yeast/rocket_yeast.py``
    (``mode='flow'``: the velocity that advects both is ``-epsilon / cs^2`` times the D2Q9 stencil over the surfactant, and the
    population feels the Shan-Chen force ``-G_chen psi grad psi``) and ``rocket_yeast_forces_only.py`` (``mode='forces'``: the
    velocity is the sum of a surface force over ``S(c)`` and a pressure force over the population).  ``run(n)`` advances both
    with one launch per time step and no host wait (``lb_run_rocket``: the stencil operands of a workgroup's rows and their halo in
    LDS; ``set_variant(0)``: two launches, the densities through memory; the same bits); the phase methods run the reference's
    stages one by one and equal it bitwise.  Arrays are shaped like the reference's, ``(nx, ny, 2[, 9])`` in Fortran order with
    the population at index 0 and the surfactant at 1; ``u``, ``v``, ``psi`` / ``S`` and the forces are ``(nx, ny)``."""
    MODES = {"flow": _native.LB_ROCKET_FLOW, "forces": _native.LB_ROCKET_FORCES}
    PARAMS = ("G", "G_c", "epsilon", "rho_o", "G_chen", "c_o", "alpha")
    _RUN, _STACKED, _SHARED = "lb_run_rocket", ("f", "feq", "rho"), ("u", "v")
    _OWN = ("psi", "S", "pseudo_force_x", "pseudo_force_y", "surface_force_x", "surface_force_y")

    def __init__(self, nx, ny, omega, omega_c, mode="flow", device=0, planar=None):
        if mode not in self.MODES:
            raise ValueError("mode must be 'flow' or 'forces'")
        self.omega, self.omega_c, self.mode = float(omega), float(omega_c), mode
        self._adopt(nx, ny, [Simulation(nx, ny, om, bc="periodic", semantics="rocket", device=device, planar=planar) for om in (omega, omega_c)])
        self.params = dict(G=0., G_c=0., epsilon=0., rho_o=1., G_chen=0., c_o=1., alpha=1.)
        self.set_params()

    def set_params(self, **kw):
        """G, G_c (growth and secretion rate per step), epsilon, rho_o, G_chen, c_o, alpha: float32, stored with the first member."""
        for k in kw:
            if k not in self.PARAMS:
                raise TypeError("unknown parameter %r (one of %s)" % (k, ", ".join(self.PARAMS)))
        self.params.update({k: float(np.float32(v)) for k, v in kw.items()})
        p = _native.RocketParams(self.MODES[self.mode], *[self.params[k] for k in self.PARAMS])
        self._call("lb_set_rocket", ct.byref(p))

    def get_params(self):
        p = _native.RocketParams()
        check(self._lib.lb_get_rocket(self.members[0]._h, ct.byref(p)))
        return dict(mode=[k for k, v in self.MODES.items() if v == p.mode][0], **{k: getattr(p, k) for k in self.PARAMS})

    def get_fields(self, which=("f", "feq", "rho", "u", "v")):
        """f, feq: (nx, ny, 2, 9); rho: (nx, ny, 2); u, v: (nx, ny); 'psi' and 'pseudo_force_x/y' (flow), 'S',
        'surface_force_x/y' and 'pseudo_force_x/y' = the pressure force (forces): (nx, ny), those of the last step."""
        return self._get_fields(which)

    def _read_own(self, own, out):
        for k in own:
            out[k] = np.zeros((self.nx, self.ny), np.float32, order="F")
        ptr = lambda *ks: next((out[k].ctypes.data for k in ks if k in out), None)
        self._call("lb_get_rocket_fields", ptr("psi", "S"), ptr("pseudo_force_x"), ptr("pseudo_force_y"),
                   ptr("surface_force_x"), ptr("surface_force_y"))
        if "psi" in out and "S" in out:
            out["S"][...] = out["psi"]

    # -- the reference's stages that involve both lattices, un-fused -----------------------------------------------------------
    def update_velocity(self):
        self._call("lb_update_velocity_rocket")
        self.sync()

    def update_forces(self):
        self._call("lb_update_forces_rocket")
        self.sync()

    def collide_particles(self):
        self._call("lb_collide_rocket")
        self.sync()

    def step_phases(self):
        """One time step as the reference's run loop makes it, stage by stage (each call waits): the velocity before the forces
        in mode 'flow', from them in mode 'forces'."""
        self.move()
        self.move_bcs()
        self.update_hydro()
        if self.mode == "flow":
            self.update_velocity()
            self.update_forces()
        else:
            self.update_forces()
            self.update_velocity()
        self.update_feq()
        self.collide_particles()

    def use_stream(self, hip_stream):
        for m in self.members:
            m.use_stream(hip_stream)

    # -- checkpoints: every member's arrays under 'm<i>_', the parameters with the first -----------------------------------------
    def _own_entries(self):
        return {"mode": np.array(self.mode), "params": np.array([self.params[k] for k in self.PARAMS], np.float32)}

    @classmethod
    def from_checkpoint(cls, path, device=0):
        own, per = cls._load_entries(path)
        # (the members' omegas as they were given: the restored colony writes the same file)
        out = cls(int(per[0]["nx"]), int(per[0]["ny"]), per[0]["omega"][()], per[1]["omega"][()], mode=str(own["mode"]), device=device)
        out.set_params(**dict(zip(cls.PARAMS, [float(x) for x in own["params"]])))
        for m, p in zip(out.members, per):
            m.restore_arrays(p)
        out.update_forces()             # psi / S and the forces of the last step follow from its densities
        return out


class Advected_Scalars(_Shared_Velocity, _Lattice_Set):
    """A flow and the concentrations it carries -- a dye, a temperature, a growing population under a live velocity field: one periodic
    flow ``Simulation`` (``semantics='opencl'``, no obstacles) and one or two periodic scalar lattices (``semantics='diffusion'``, their
    own ``omega`` and ``G``) of its grid and device, made of existing objects, which stay their owners'.  ``run(n)`` advances all of
    them in lock step without a host wait (``lb_run_advected``): in every step each scalar is advected by the velocity the flow's
    step forms from its streamed populations -- what an ``eager_macro=True`` flow stores --, handed from the flow's collision to the
    scalars' in registers (``form=1``: one launch per step) or read from the flow's own u, v planes (``form=0``: one launch per
    lattice, no copy); the same bits, and those of ``flow.run(1)`` / ``s.set_velocity_from(flow)`` / ``s.run(1)`` step by step.
    ``members`` holds the scalars, ``flow`` the flow beside them.  Afterwards the flow's rho, u, v are stored (also on a handle that
    otherwise rebuilds them on demand) and every scalar's u, v hold the last step's velocity.  The set has no state of its own."""
    MAX_SCALARS = 2
    _STACKED, _SHARED = ("f", "feq", "rho"), ("u", "v")
    _FLOW_KEYS = {"rho_flow": "rho", "f_flow": "f", "feq_flow": "feq"}

    def __init__(self, flow, scalars):
        scalars = list(scalars)
        if not 1 <= len(scalars) <= self.MAX_SCALARS:
            raise ValueError("1..%d scalars are built (got %d)" % (self.MAX_SCALARS, len(scalars)))
        if flow.semantics != "opencl":
            raise ValueError("the flow must have semantics='opencl' (got %r)" % (flow.semantics,))
        if flow.bc_mode != _native.LB_BC_PERIODIC:
            raise ValueError("the flow must have bc='periodic': the scalar lattice has no wall rule")
        if flow.local_ny != flow.ny:
            raise ValueError("the flow must own its whole grid")
        for i, s in enumerate(scalars):
            if s.semantics != "diffusion":
                raise ValueError("scalar %d must have semantics='diffusion' (got %r)" % (i, s.semantics))
            if s.bc_mode != _native.LB_BC_PERIODIC:
                raise ValueError("scalar %d must have bc='periodic'" % i)
            if (s.nx, s.ny) != (flow.nx, flow.ny):
                raise ValueError("scalar %d has a %dx%d grid, the flow %dx%d" % (i, s.nx, s.ny, flow.nx, flow.ny))
            if s.device != flow.device:
                raise ValueError("scalar %d is on device %d, the flow on %d" % (i, s.device, flow.device))
            if any(s is t for t in scalars[:i]):
                raise ValueError("scalar %d appears twice" % i)
        self.flow = flow
        self._adopt(flow.nx, flow.ny, scalars)

    def close(self):
        self.flow.close()
        _Lattice_Set.close(self)

    def sync(self):
        self.flow.sync()
        _Lattice_Set.sync(self)

    def use_stream(self, hip_stream):
        """The stream everything is enqueued on is the flow's; the scalars' own streams are joined and released."""
        self.flow.use_stream(hip_stream)

    # -- the hot path ---------------------------------------------------------------------------------------------------------
    def run(self, num_iterations, wait=True, form=-1):
        """num_iterations time steps of the flow and every scalar; form 1: one launch per step, 0: one per lattice, -1: the planner's."""
        check(self._lib.lb_run_advected(self.flow._h, self._handles, self.num_populations, int(num_iterations), int(form)))
        if wait:
            self.sync()

    def hot_kernel(self, form=-1):
        """Name of what run(form=form) launches for this grid and number of scalars (lb_advected_kernel)."""
        buf = ct.create_string_buffer(512)
        check(self._lib.lb_advected_kernel(self.num_populations, int(form), self.nx * self.ny, buf, len(buf)))
        return buf.value.decode()

    def get_fields(self, which=("f", "rho", "u", "v", "rho_flow")):
        """f: (nx, ny, NS, 9) and rho: (nx, ny, NS) of the scalars; u, v: (nx, ny), the flow's; rho_flow, f_flow, feq_flow: the flow's."""
        out = self._get_fields(tuple(k for k in which if k in self._STACKED))
        keys = tuple(k for k in which if k in self._SHARED) + tuple(v for k, v in self._FLOW_KEYS.items() if k in which)
        if keys:
            g = self.flow.get_fields(keys)
            out.update({k: g[k] for k in self._SHARED if k in which})
            out.update({k: g[v] for k, v in self._FLOW_KEYS.items() if k in which})
        return out

    def check(self):
        """{'flow': the flow's Simulation.check(), 'scalars': [every scalar's]}."""
        return {"flow": self.flow.check(), "scalars": _Shared_Velocity.check(self)}

    # -- checkpoints: every scalar's arrays under 'm<i>_', the flow's under 'flow_' ---------------------------------------------------
    def save_checkpoint(self, path):
        own = {"flow_" + k: a for k, a in self.flow.checkpoint_arrays().items()}
        own["flow_eager_macro"] = int(self.flow.eager_macro)
        np.savez(Simulation._ckpt_path(path), **dict(own, **self._member_entries()))

    @classmethod
    def from_checkpoint(cls, path, device=0):
        own, per = cls._load_entries(path)
        d = {k[len("flow_"):]: a for k, a in own.items() if k.startswith("flow_")}
        # (omegas as they were given: the restored set writes the same file)
        flow = Simulation(int(d["nx"]), int(d["ny"]), d["omega"][()], bc=int(d["bc_mode"]), inlet_rho=float(d["inlet_rho"]),
                          outlet_rho=float(d["outlet_rho"]), lid_u=float(d["lid_u"]), rho0=float(d["rho0"]), device=device,
                          semantics=str(d["semantics"]), inlet_u=float(d["inlet_u"]), outlet_u=float(d["outlet_u"]),
                          eager_macro=bool(int(d["eager_macro"])))
        flow.restore_arrays(d)
        scalars = []
        for p in per:
            s = Simulation(int(p["nx"]), int(p["ny"]), p["omega"][()], bc=int(p["bc_mode"]), device=device, semantics=str(p["semantics"]))
            s.restore_arrays(p)
            scalars.append(s)
        return cls(flow, scalars)
