"""The forces-only variant of the surfactant-propelled colony: the surface of the reference's
``LB_D2Q9.rocket_yeast.rocket_yeast_forces_only`` (class ``Rocket_Yeast_Forces_Only``) on a pair of rocket handles of liblbhip
(``LB_D2Q9.coupled.Surfactant_Colony(..., mode='forces')``).

The velocity is the sum of two forces: the surface force ``-epsilon / cs^2 grad S`` over the coverage
``S = (1 - exp(-c / c_o))^alpha`` and the pressure force ``-G_chen / cs^2 grad rho (rho - rho_o)`` over the population (kept under
the reference's name, ``pseudo_force_x/y``); the population does not grow where its density exceeds 1.  Unlike ``Rocket_Yeast``
this class rounds ``delta_x`` and ``delta_t`` to float32 before deriving the other constants.  Everything else is as in
``LB_D2Q9.rocket_yeast.rocket_yeast``, differences included.
"""
import numpy as np

from .rocket_yeast import Rocket_Yeast, cs, cx, cy, w  # noqa: F401


class Rocket_Yeast_Forces_Only(Rocket_Yeast):
    _MODE = "forces"
    _KEYS = ("rho", "f", "feq", "u", "v", "S", "surface_force_x", "surface_force_y", "pseudo_force_x", "pseudo_force_y")

    def __init__(self, Lx=1.0, Ly=1.0, R0=5., epsilon=1., Dc=1. / 4., Gc=2.0, rho_o=1.0, c_o=0.25, alpha=2.0, G_chen=-1.0,
                 time_prefactor=1., N=10, two_d_local_size=(32, 32), use_interop=False, check_max_ulb=False, mach_tolerance=0.1,
                 rng=None, device=0, verbose=False):
        Rocket_Yeast.__init__(self, Lx=Lx, Ly=Ly, R0=R0, epsilon=epsilon, Dc=Dc, Gc=Gc, rho_o=rho_o, G_chen=G_chen,
                              time_prefactor=time_prefactor, N=N, two_d_local_size=two_d_local_size, use_interop=use_interop,
                              check_max_ulb=check_max_ulb, mach_tolerance=mach_tolerance, rng=rng, device=device, verbose=verbose,
                              c_o=c_o, alpha=alpha)
        self.psi = None                                 # (the reference's attribute: never filled by this class)

    def _more_parameters(self, c_o=0.25, alpha=2.0):
        self.c_o, self.alpha = np.float32(c_o), np.float32(alpha)

    def _discretization(self, N, time_prefactor):
        delta_x = np.float32(1. / N)
        return delta_x, np.float32(time_prefactor * np.float64(delta_x) ** 2)

    def _engine_params(self):
        return dict(Rocket_Yeast._engine_params(self), c_o=self.c_o, alpha=self.alpha)

    def _stage_three(self):
        self.update_forces()
        self.update_u_and_v()

    def update_forces(self):
        self._engine.update_forces()

    update_force = update_forces
