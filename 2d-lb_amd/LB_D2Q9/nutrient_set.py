"""A population and the nutrient it eats, advected by a velocity solved from the population: two scalar lattices
(``Simulation(semantics='diffusion', bc='periodic')``, ``omega`` and ``omega_n``) and a spectral screened-Poisson solver
(``spectral_poisson.Screened_Poisson``) on one periodic grid -- the engine under
``reaction_diffusion.surfactant_nutrient_waves``.

Per step the population's density after streaming is solved for ``(1 - lam^2 laplace) phi = rho_p``, ``(u, v) = scale Re grad phi``
advects both lattices, the population gains ``w_k G rho_p rho_n`` and the nutrient loses it; ``clumpy`` adds the Shan-Chen
self-attraction ``F = -cs^2 G_chen psi grad_w psi`` on the population.  ``run(n)`` is five launches per step and no host wait
(``lb_run_nutrient``); the phase methods run the reference's stages one by one.  No handle kind of its own: the parameters travel
with every call, ``psi`` and the force live with the first member.  Arrays are shaped like the reference's, ``(nx, ny, 2[, 9])`` in
Fortran order with the population at index 0 and the nutrient at 1; ``u``, ``v``, ``psi`` and the force are ``(nx, ny)``.
"""
import ctypes as ct

import numpy as np

from . import _native
from ._native import check
from .coupled import _Lattice_Set, _Shared_Velocity
from .simulation import Simulation
from .spectral_poisson.screened_poisson import Screened_Poisson


class Nutrient_Set(_Shared_Velocity, _Lattice_Set):
    PARAMS = ("G", "scale", "clumpy", "rho_o", "G_chen")
    _STACKED, _SHARED, _OWN = ("f", "feq", "rho"), ("u", "v"), ("psi", "pseudo_force_x", "pseudo_force_y")

    def __init__(self, nx, ny, omega, omega_n, lam=1., dx=1., device=0, planar=None):
        self.omega, self.omega_n = float(omega), float(omega_n)
        # (the solver first: a length that is not 2^a 3^b 5^c <= 4096 is refused before a device is touched)
        self.solver = Screened_Poisson(np.zeros((int(nx), int(ny)), np.complex64, order="F"), lam=lam, dx=dx, device=device)
        self.solver.create_grad_fields()
        self._adopt(nx, ny, [Simulation(nx, ny, om, bc="periodic", semantics="diffusion", device=device, planar=planar)
                             for om in (omega, omega_n)])
        self.params = dict(G=0., scale=0., clumpy=False, rho_o=1., G_chen=0.)

    def close(self):
        _Lattice_Set.close(self)
        self.solver.close()

    def set_params(self, **kw):
        """G (growth per step), scale (the factor on Re grad phi), clumpy, rho_o, G_chen: float32, kept here and sent with every call."""
        for k in kw:
            if k not in self.PARAMS:
                raise TypeError("unknown parameter %r (one of %s)" % (k, ", ".join(self.PARAMS)))
        self.params.update({k: bool(v) if k == "clumpy" else float(np.float32(v)) for k, v in kw.items()})

    def _params(self):
        p = self.params
        return ct.byref(_native.NutrientParams(p["G"], p["scale"], int(p["clumpy"]), p["rho_o"], p["G_chen"]))

    # -- the hot path ---------------------------------------------------------------------------------------------------------
    def run(self, num_iterations, wait=True):
        """num_iterations fused time steps of both members, five launches per step."""
        check(self._lib.lb_run_nutrient(self.solver._h, self._handles, 2, self._params(), int(num_iterations)))
        if wait:
            self.sync()

    # -- the reference's stages that involve both lattices, un-fused --------------------------------------------------------------
    def update_velocity(self, streamed=False):
        """(u, v) = scale Re grad phi of the population's stored rho (streamed: of its density after streaming), into both members."""
        check(self._lib.lb_nutrient_velocity(self.solver._h, self._handles, 2, self.params["scale"], int(bool(streamed))))
        self.sync()

    def update_forces(self):
        if self.params["clumpy"]:
            self._call("lb_update_forces_nutrient", self._params())
            self.sync()

    def collide_particles(self):
        self._call("lb_collide_nutrient", self._params())
        self.sync()

    def step_phases(self):
        """One time step as the reference's run loop makes it, stage by stage (each call waits)."""
        self.move()
        self.move_bcs()
        self.update_hydro()
        self.update_velocity()
        self.update_forces()
        self.update_feq()
        self.collide_particles()

    def get_fields(self, which=("f", "feq", "rho", "u", "v")):
        """f, feq: (nx, ny, 2, 9); rho: (nx, ny, 2); u, v: (nx, ny); 'psi', 'pseudo_force_x/y' (clumpy): (nx, ny), the last step's."""
        return self._get_fields(which)

    def _read_own(self, own, out):
        for k in own:
            out[k] = np.zeros((self.nx, self.ny), np.float32, order="F")
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._call("lb_get_nutrient_fields", ptr("psi"), ptr("pseudo_force_x"), ptr("pseudo_force_y"))

    def use_stream(self, hip_stream):
        for m in self.members:
            m.use_stream(hip_stream)
