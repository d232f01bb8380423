"""A Fisher wave that advects itself: the surface of the reference's ``LB_D2Q9.reaction_diffusion.screened_poisson_waves``
(``Screened_Fisher_Wave``) on a scalar-lattice handle of liblbhip (``Simulation(..., semantics='diffusion', bc='open')``) and an
``lb_spectral`` (``spectral_poisson.Screened_Poisson``).

The lattice is ``diffusion.Reaction_Diffusion``'s -- linear equilibrium, growth ``w_k G rho (1 - rho)`` -- with a velocity that is
no longer imposed: every step solves ``(1 - lam^2 laplace) phi = rho`` in the periodic box and sets
``(u, v) = -vc (delta_t / delta_x) Re grad phi``.  ``run(n)`` is fused HIP -- per step one launch for the density after streaming,
three for the solve, one for the step, no host wait (lb_run_screened) -- where the reference makes some twenty launches and array
passes and waits after each; the phase methods run the reference's sequence un-fused.

Everything is in dimensionless units: ``L = T = 1``, ``D = 1/4``, ``G = 1``.  The parameter arithmetic lives in
``screened_fisher_parameters`` and needs no handle.  Repairs: ``np.float`` no longer exists; the Gaussian of
``init_hydro`` is laid out with ``indexing='ij'`` so that boxes that are not square work (identical where the reference runs);
``nx / 2`` is the integer ``nx // 2`` it was under Python 2; ``init_pop(perturb=None)`` takes the perturbation as an argument;
``check_max_ulb`` goes through the engine's health check (lb_check's largest Mach number) and is made after ``run`` as well.
Grid sizes must be ``2^a 3^b 5^c <= 4096`` on each axis (the transform's lengths).
"""
import numpy as np

from .. import _native
from .._dropin import NUM_JUMPERS, DeviceField, DropIn, get_divisible_global, lattice_arrays  # noqa: F401
from .._native import check
from ..simulation import Simulation
from ..spectral_poisson import screened_poisson as sp

w, cx, cy = lattice_arrays(np.float32, np.int32)
cs = np.float32(1. / np.sqrt(3))


# ---- parameter arithmetic: no handle, no GPU -----------------------------------------------------------------------
def screened_fisher_parameters(Lx=1.0, Ly=1.0, vc=1., time_prefactor=1., N=50):
    """delta_x = 1 / N, delta_t = time_prefactor delta_x^2; D = 1/4 and G = 1 in lattice units, the relaxation rate, the grid
    (round(N Lx), round(N Ly): no boundary nodes are added) and the factor between Re grad phi and the lattice velocity."""
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    lb_D = np.float32(.25 * (delta_t / delta_x ** 2))
    omega = np.float32((.5 + lb_D / cs ** 2) ** -1.)
    assert omega < 2.
    return dict(N=N, delta_x=delta_x, delta_t=delta_t, ulb=delta_t / delta_x, D=.25, G=1., lb_D=lb_D, omega=omega,
                lb_G=np.float32(1. * delta_t), nx=int(np.round(N * Lx)), ny=int(np.round(N * Ly)),
                velocity_scale=-vc * (delta_t / delta_x))


def gaussian_droplet(nx, ny, N, R0):
    """rho = exp(-(X^2 + Y^2) / R0^2) around (nx // 2, ny // 2), X, Y in units of the characteristic length; (nx, ny) arrays."""
    x_center, y_center = nx // 2, ny // 2
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    X_dim = (X.astype(np.float64) - x_center) / N
    Y_dim = (Y.astype(np.float64) - y_center) / N
    rho = np.asfortranarray(np.exp(-(X_dim ** 2 + Y_dim ** 2) / R0 ** 2).astype(np.float32))
    return x_center, y_center, X_dim, Y_dim, rho


class Screened_Fisher_Wave(DropIn):
    """Everything is in dimensionless units."""

    _sim = property(lambda self: self.sim)      # the engine under the name the shared methods use

    def __init__(self, Lx=1.0, Ly=1.0, vc=1., lam=1., R0=5., time_prefactor=1., N=50,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False,
                 check_max_ulb=False, mach_tolerance=0.1, device=0):
        self.Lx, self.Ly = Lx, Ly
        self.D, self.G = 1. / 4., 1.
        self.vc, self.lam, self.R0 = vc, lam, R0
        self.use_interop = use_interop
        self.check_max_ulb, self.mach_tolerance = check_max_ulb, mach_tolerance
        self.L = self.T = 1.0

        p = screened_fisher_parameters(Lx=Lx, Ly=Ly, vc=vc, time_prefactor=time_prefactor, N=N)
        self.N, self.delta_x, self.delta_t, self.ulb = p["N"], p["delta_x"], p["delta_t"], p["ulb"]
        print('u_lb:', self.ulb)
        self.lb_D, self.omega, self.lb_G = p["lb_D"], p["omega"], p["lb_G"]
        print('omega', self.omega)
        self.nx, self.ny = p["nx"], p["ny"]
        self.velocity_scale = np.float32(p["velocity_scale"])

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)

        self._lib = _native.lib()
        self.sim = Simulation(self.nx, self.ny, self.omega, bc="open", semantics="diffusion", device=device)
        self.sim.set_reaction(self.lb_G)
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")

        self.x_center = self.y_center = self.X = self.Y = None
        self.poisson_solver = None
        self.init_hydro(device)
        self.update_feq()
        self.init_pop()

    # -- state -----------------------------------------------------------------------------------------------------------
    def _set_rho(self, rho):
        zero = np.zeros((self.nx, self.ny), dtype=np.float32, order='F')
        self.sim.set_fields(rho, zero, zero)

    def init_hydro(self, device=0):
        """The Gaussian droplet, the Poisson solver, and the velocity the droplet gives itself."""
        self.x_center, self.y_center, self.X, self.Y, rho = gaussian_droplet(self.nx, self.ny, self.N, self.R0)
        self._set_rho(rho)
        self.poisson_solver = sp.Screened_Poisson(rho, lam=self.lam, dx=self.delta_x, device=device)
        self.poisson_solver.create_grad_fields()
        self.update_u_and_v()

    def redo_initial_condition(self, rho_field):
        """After you have specified your own initial condition."""
        self._set_rho(np.asarray(rho_field).astype(np.float32, order='F'))
        self.update_u_and_v()
        self.update_feq()
        self.init_pop()

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb; None = exactly feq (the reference's amplitude 0)."""
        self.sim.init_pop(perturb)

    def _check_ulb(self):
        if self.check_max_ulb:
            mach = self.sim.check()["max_mach"]
            if mach > self.mach_tolerance:
                print('max_ulb is greater than cs/10! Ma=', mach)

    # -- the phases ------------------------------------------------------------------------------------------------------
    def update_u_and_v(self):
        """(u, v) = -vc (delta_t / delta_x) Re grad phi of the stored rho: three launches (lb_spectral_velocity)."""
        check(self._lib.lb_spectral_velocity(self.poisson_solver._h, self.sim._h, float(self.velocity_scale), 0))
        self.sim.sync()
        self._check_ulb()

    def update_hydro(self):
        self.sim.update_hydro()
        self.update_u_and_v()

    def run(self, num_iterations):
        """num_iterations time steps, fused on the device; returns with the work complete."""
        check(self._lib.lb_run_screened(self.poisson_solver._h, self.sim._h, float(self.velocity_scale), int(num_iterations)))
        self.sim.sync()
        self._check_ulb()

    def step(self):
        self.run(1)
