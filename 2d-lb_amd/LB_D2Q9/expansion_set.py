"""Noisy strains on a shared nutrient: one to three populations that each grow on, and deplete, one nutrient lattice, advected by one
imposed velocity field -- the engine under ``advecting_range_expansion.stochastic_nutrients``.

Every strain is one scalar lattice with the noisy collision (``NoisySimulation``, its own ``omega``, ``G``, ``Dg`` and seed), the nutrient
one plain scalar lattice (``Simulation(semantics='diffusion')``, ``omega_nutrient``), all in one box: ``bc='open'`` is the reference's
box (a link that would enter from outside keeps the member's edge state), ``bc='periodic'`` wraps.  Per step every member streams,
``rho_i = sum f_ik`` is cut to 0 below ``zero_cutoff``, and with ``c`` the nutrient's density strain i gains
``w_k ((G_i rho_i) c + sqrt((Dg_i rho_i) c) z_i + ((Dg_i c) / 4)(z_i^2 - 1))`` -- growth, multiplicative demographic noise and its
Milstein correction -- while the nutrient loses the sum; a link that would fall below 0 becomes 0.  ``run(n)`` is ONE launch per step
and no host wait (``lb_run_expansion``): the normals are drawn inside the kernel from each strain's counter-based stream.  The phase
methods run the reference's stages one by one.  No handle kind of its own: ``zero_cutoff`` travels with every call.  Arrays are shaped
like the reference's, ``(nx, ny, NP + 1[, 9])`` in Fortran order with the nutrient last; ``u``, ``v`` are ``(nx, ny)``.
"""
import ctypes as ct

import numpy as np

from . import _native
from ._native import check
from .coupled import _Lattice_Set, _Shared_Velocity
from .noisy_simulation import NoisySimulation
from .simulation import Simulation


class Expansion_Set(_Shared_Velocity, _Lattice_Set):
    MAX_STRAINS = 3
    _STACKED, _SHARED = ("f", "feq", "rho"), ("u", "v")

    def __init__(self, nx, ny, omegas, omega_nutrient, Gs, bc="open", zero_cutoff=0.01, device=0, planar=None):
        omegas, Gs = [float(o) for o in np.atleast_1d(omegas)], [float(g) for g in np.atleast_1d(Gs)]
        if not 1 <= len(omegas) <= self.MAX_STRAINS:
            raise ValueError("1..%d strains are built (got %d)" % (self.MAX_STRAINS, len(omegas)))
        if len(Gs) != len(omegas):
            raise ValueError("one omega and one G per strain")
        if bc not in ("open", "periodic"):
            raise ValueError("bc must be 'open' or 'periodic'")
        self.omegas, self.omega_nutrient, self.Gs, self.bc = omegas, float(omega_nutrient), Gs, bc
        self.zero_cutoff = float(np.float32(zero_cutoff))
        self.num_strains = len(omegas)
        members = [NoisySimulation(nx, ny, om, bc=bc, device=device, planar=planar) for om in omegas]
        members.append(Simulation(nx, ny, omega_nutrient, bc=bc, semantics="diffusion", device=device, planar=planar))
        self._adopt(nx, ny, members)
        for m, g in zip(self.strains, Gs):
            m.set_reaction(g)

    @property
    def strains(self):
        return self.members[:-1]

    @property
    def nutrient(self):
        return self.members[-1]

    def _params(self):
        return ct.byref(_native.ExpansionParams(self.zero_cutoff))

    # -- the noise ------------------------------------------------------------------------------------------------------------
    def set_noise(self, Dgs, seed=0):
        """Strain i draws under ``seed + i`` with strength ``Dgs[i]`` (a scalar: the same for all); every noise counter restarts at 0.
        ``Dg == 0`` switches a strain's noise off: it draws nothing and its counter does not move."""
        Dgs = np.broadcast_to(np.asarray(Dgs, np.float64), (self.num_strains,))
        for i, m in enumerate(self.strains):
            m.set_noise(float(Dgs[i]), int(seed) + i)

    def noise(self):
        """[(Dg, seed, t)] per strain: t = the noise counter, the number of noisy collisions since set_noise."""
        return [m.noise() for m in self.strains]

    # -- the hot path ---------------------------------------------------------------------------------------------------------
    def run(self, num_iterations, wait=True):
        """num_iterations fused time steps of all members, one launch per step."""
        self._call("lb_run_expansion", self._params(), int(num_iterations))
        if wait:
            self.sync()

    # -- the reference's stages that involve the whole set, un-fused ----------------------------------------------------------------
    def update_hydro(self):
        self._call("lb_update_hydro_expansion", self._params())
        self.sync()

    def collide_particles(self):
        self._call("lb_collide_expansion", self._params())
        self.sync()

    def step_phases(self):
        """One time step as the reference's run loop makes it, stage by stage (each call waits)."""
        self.move()
        self.move_bcs()
        self.update_hydro()
        self.update_feq()
        self.collide_particles()

    def get_fields(self, which=("f", "feq", "rho", "u", "v")):
        """f, feq: (nx, ny, NP + 1, 9); rho: (nx, ny, NP + 1), the nutrient last; u, v: (nx, ny) (the first member's)."""
        return self._get_fields(which)

    # -- the open box's edge state, per member ------------------------------------------------------------------------------------
    def get_edge_state(self):
        """(NP + 1, 6 (nx + ny)): every member's links that enter from outside the box (include/lb_hip.h); (NP + 1, 0) when periodic."""
        return np.stack([m.get_edge_state() for m in self.members])

    def set_edge_state(self, values):
        values = np.asarray(values, np.float32)
        if values.ndim != 2 or values.shape[0] != self.num_populations:
            raise ValueError("edge state = (NP + 1, 6 (nx + ny)) floats")
        for m, v in zip(self.members, values):
            m.set_edge_state(v)

    def use_stream(self, hip_stream):
        for m in self.members:
            m.use_stream(hip_stream)

    # -- checkpoints: every member's arrays under 'm<i>_' (the noise triple and the edge state travel with a member) ------------------
    def save_checkpoint(self, path):
        own = {"zero_cutoff": np.float32(self.zero_cutoff), "bc": np.array(self.bc)}
        np.savez(Simulation._ckpt_path(path), **dict(own, **self._member_entries()))

    @classmethod
    def from_checkpoint(cls, path, device=0):
        own, per = cls._load_entries(path)
        # (the members' omegas as they were given: the restored set writes the same file)
        out = cls(int(per[0]["nx"]), int(per[0]["ny"]), [p["omega"][()] for p in per[:-1]], per[-1]["omega"][()],
                  [0.] * (len(per) - 1), bc=str(own["bc"]), zero_cutoff=float(own["zero_cutoff"]), device=device)
        for m, p in zip(out.members, per):
            m.restore_arrays(p)
        out.Gs = [float(getattr(m, "G", 0.)) for m in out.strains]
        return out
