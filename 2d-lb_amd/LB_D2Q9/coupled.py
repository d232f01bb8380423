"""Coupled scalar lattices: several concentrations on one grid that share an imposed velocity field and compete for room.

The reference's ``advecting_range_expansion`` fork (``D2Q9_multifield_fisher.cl``) keeps ``num_populations`` fields in
arrays shaped ``(nx, ny, num_populations[, 9])`` (Fortran order) and loops over them in every work-item of five launches
per step.  Here every field is one engine lattice (``Simulation(semantics='multifield')``, its own ``omega`` and ``G``) and
``run(n)`` advances all of them with ONE fused launch per time step (``lb_run_coupled``): per cell, field i relaxes
towards ``w_k rho_i (1 + 3 c_k.u)`` and grows by ``w_k G_i rho_i (1 - sum_j rho_j)``.  ``bc='box'`` is the fork's closed
box (on-node bounce-back on all four walls), ``bc='periodic'`` wraps.  The phase methods run the fork's kernels one by
one.  The velocity the fused step reads is the first member's; ``set_fields`` / ``set_velocity_from`` write every member.
"""
import ctypes as ct

import numpy as np

from . import _native
from ._native import check
from .simulation import NUM_JUMPERS, Simulation


class Coupled_Scalars(object):
    MAX_POPULATIONS = 4

    def __init__(self, nx, ny, omegas, Gs, bc="box", device=0, planar=None):
        omegas, Gs = [float(o) for o in np.atleast_1d(omegas)], [float(g) for g in np.atleast_1d(Gs)]
        if not 1 <= len(omegas) <= self.MAX_POPULATIONS or len(Gs) != len(omegas):
            raise ValueError("1..%d fields, one omega and one G each" % self.MAX_POPULATIONS)
        if bc not in ("box", "periodic"):
            raise ValueError("bc must be 'box' or 'periodic'")
        self.nx, self.ny, self.num_populations, self.num_jumpers = int(nx), int(ny), len(omegas), NUM_JUMPERS
        self.omegas, self.Gs, self.bc = omegas, Gs, bc
        self.members = [Simulation(nx, ny, om, bc=bc, semantics="multifield", device=device, planar=planar) for om in omegas]
        for m, g in zip(self.members, Gs):
            m.set_reaction(g)
        self._lib = _native.lib()
        self._handles = (ct.c_void_p * len(omegas))(*[m._h for m in self.members])

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

    def set_fields(self, rho, u, v):
        """rho: (nx, ny, num_populations); u, v: (nx, ny), written to every member."""
        rho = self._per_field(rho)
        for i, m in enumerate(self.members):
            m.set_fields(rho[:, :, i], u, v)

    def set_velocity_from(self, flow):
        """u, v of a flow Simulation of the same grid become every member's imposed velocity, device to device."""
        for m in self.members:
            m.set_velocity_from(flow)

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb on every member; perturb None or (nx, ny, num_populations, 9)."""
        for i, m in enumerate(self.members):
            m.init_pop(None if perturb is None else np.asarray(perturb)[:, :, i, :])

    def get_fields(self, which=("f", "feq", "u", "v", "rho")):
        """f, feq: (nx, ny, num_populations, 9); rho: (nx, ny, num_populations); u, v: (nx, ny) (the first member's)."""
        out = {}
        stacked = [k for k in which if k in ("f", "feq", "rho")]
        if stacked:
            per = [m.get_fields(tuple(stacked)) for m in self.members]
            for k in stacked:
                out[k] = np.asfortranarray(np.stack([g[k] for g in per], axis=2))
        shared = tuple(k for k in which if k in ("u", "v"))
        if shared:
            out.update(self.members[0].get_fields(shared))
        return out

    def get_corner_state(self):
        """(num_populations, 8): every member's never-written corner links (bc='box'; include/lb_hip.h)."""
        return np.stack([m.get_corner_state() for m in self.members])

    def set_corner_state(self, values):
        values = np.asarray(values, np.float32)
        if values.shape != (self.num_populations, 8):
            raise ValueError("corner state = (num_populations, 8) floats")
        for m, v in zip(self.members, values):
            m.set_corner_state(v)

    # -- the fork's phases, un-fused ------------------------------------------------------------------------------------
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

    def collide_particles(self):
        check(self._lib.lb_collide_coupled(self._handles, self.num_populations))
        self.sync()

    # -- the hot path ---------------------------------------------------------------------------------------------------
    def run(self, num_iterations, wait=True):
        """num_iterations fused time steps of all fields, one launch per step."""
        check(self._lib.lb_run_coupled(self._handles, self.num_populations, int(num_iterations)))
        if wait:
            self.sync()

    def step(self):
        self.run(1)

    def check(self):
        """Per member: Simulation.check() (non-finite cells, max Mach number of the imposed field, sum of rho)."""
        return [m.check() for m in self.members]
