"""Fisher waves with demographic noise: the surface of the reference's ``LB_D2Q9.reaction_diffusion.noisy_fisher_wave``
(``Noisy_Advected_Fisher_Wave``) on a scalar-lattice handle of liblbhip with the noisy collision switched on
(``LB_D2Q9.noisy_simulation.NoisySimulation``).

The collision adds ``w_k (G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z)`` and sets a link that went negative to zero; ``z`` is a
standard normal per cell and step.  The reference keeps the normals in a buffer that pyopencl's ``PhiloxGenerator.fill_normal``
refills between steps, unseeded, with a host wait each time; here the kernels draw them in registers from a counter-based stream
(Philox4x32-10 under ``seed``: csrc/philox.h) -- a sequence of its own, not pyopencl's, and reproducible: the same ``seed`` gives
the same run, however ``run`` is split.  As in the reference, a density outside [0, 1] makes the square root NaN.

Two arguments beyond the reference's: ``seed=0`` and ``perturb=None`` (what ``Diffusion.init_pop`` takes: the reference multiplies
the populations by 1 + 0.001 randn, unseeded; None = exactly feq).  The reference's default ``vc=0`` divides by zero in
``init_hydro`` (``Pe * vx / vc``): kept -- pass a ``vc``.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, DropIn, get_divisible_global  # noqa: F401
from ..noisy_simulation import NoisySimulation
from .diffusion import gaussian_blob, grid_dims, lattice_discretisation, omega_of


def noisy_fisher_parameters(Lx=1.0, Ly=1.0, D=1.0, z=0.1, vx=0., vy=0., vc=0., g=1.0, Nc=10., time_prefactor=1., N=50):
    """The derived numbers of the class (noisy_fisher_wave.py:188-230), no handle: L = z, T = z^2 / D, Pe = z vc / D,
    dim_Gd = g z^2 / D, lb_Gd = dim_Gd delta_t, Dg = (1 / Nc) (z / D), lb_Dg = Dg delta_t / delta_x, lb_D = delta_t / delta_x^2.
    The lattice velocity (delta_t / delta_x) Pe (vx, vy) / vc is left to the class: it divides by vc."""
    p = dict(L=z, T=z ** 2 / D)
    p.update(lattice_discretisation(N, time_prefactor))
    p["Pe"] = z * vc / D
    p["dim_Gd"] = g * z ** 2 / D
    p["lb_Gd"] = np.float32(p["dim_Gd"] * p["delta_t"])
    p["Dg"] = (1. / Nc) * (z / D)
    p["lb_Dg"] = np.float32(p["Dg"] * p["delta_t"] / p["delta_x"])
    p["dim_D"] = 1.0
    p["lb_D"] = np.float32(p["dim_D"] * (p["delta_t"] / p["delta_x"] ** 2))
    p["omega"] = np.float32(omega_of(p["lb_D"]))
    p.update(grid_dims(Lx, Ly, p["L"], N))
    return p


class Noisy_Advected_Fisher_Wave(DropIn):
    _bc = "open"       # the reference's box: move_bcs does nothing
    _sim = property(lambda self: self.sim)

    def __init__(self, Lx=1.0, Ly=1.0, D=1.0, z=0.1, vx=0., vy=0., vc=0., g=1.0, Nc=10., time_prefactor=1., N=50,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False, seed=0, perturb=None, device=0):
        self.phys_Lx, self.phys_Ly, self.phys_D, self.phys_z = Lx, Ly, D, z
        self.phys_vx, self.phys_vy, self.phys_vc = vx, vy, vc
        self.phys_g, self.phys_Nc = g, Nc
        self.use_interop, self.seed, self.time_prefactor = use_interop, int(seed), time_prefactor

        self.L = self.T = None
        self.set_characteristic_length_time()
        print('Characteristic L:', self.L)
        print('Characteristic T:', self.T)

        d = lattice_discretisation(N, time_prefactor)
        self.N, self.delta_x, self.delta_t, self.ulb = d["N"], d["delta_x"], d["delta_t"], d["ulb"]
        print('u_lb:', self.ulb)

        self.lb_D = self.omega = self.dim_D = self.Pe = None
        self.dim_Gd = self.lb_Gd = self.Dg = self.lb_Dg = None
        self.set_pde_constants()

        self.lx = self.ly = self.nx = self.ny = None
        self.initialize_grid_dims()

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)
        print('2d global:', self.two_d_global_size)
        print('2d local:', self.two_d_local_size)
        print('3d global:', self.three_d_global_size)
        print('3d local:', self.three_d_local_size)

        self.sim = NoisySimulation(self.nx, self.ny, self.omega, bc=self._bc, device=device)
        self.sim.set_reaction(self.lb_Gd)
        self.sim.set_noise(self.lb_Dg, self.seed)
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")

        self.x_center = self.y_center = self.X_dim = self.Y_dim = None
        self.init_hydro()
        self.update_feq()
        self.init_pop(perturb)

    def set_pde_constants(self):
        p = noisy_fisher_parameters(Lx=self.phys_Lx, Ly=self.phys_Ly, D=self.phys_D, z=self.phys_z, vx=self.phys_vx, vy=self.phys_vy,
                                    vc=self.phys_vc, g=self.phys_g, Nc=self.phys_Nc, time_prefactor=self.time_prefactor,
                                    N=self.N)
        self.Pe, self.dim_Gd, self.lb_Gd, self.Dg, self.lb_Dg = p["Pe"], p["dim_Gd"], p["lb_Gd"], p["Dg"], p["lb_Dg"]
        self.dim_D, self.lb_D, self.omega = p["dim_D"], p["lb_D"], p["omega"]
        print('Pe:', self.Pe)
        print('dim_Gd:', self.dim_Gd)
        print('Dg:', self.Dg)
        print('omega', self.omega)

    def set_characteristic_length_time(self):
        self.L = self.phys_z
        self.T = self.phys_z ** 2 / self.phys_D

    def initialize_grid_dims(self):
        g = grid_dims(self.phys_Lx, self.phys_Ly, self.L, self.N)
        self.lx, self.ly, self.nx, self.ny = g["lx"], g["ly"], g["nx"], g["ny"]

    def init_hydro(self):
        """A Gaussian blob around (nx // 2, ny // 2) and the uniform velocity (delta_t / delta_x) Pe (vx, vy) / vc."""
        self.x_center, self.y_center, self.X_dim, self.Y_dim, rho = gaussian_blob(self.nx, self.ny, self.N)
        dim_vx = self.Pe * self.phys_vx / self.phys_vc          # (vc = 0, the reference's default: ZeroDivisionError, as there)
        dim_vy = self.Pe * self.phys_vy / self.phys_vc
        lb_vx, lb_vy = (self.delta_t / self.delta_x) * dim_vx, (self.delta_t / self.delta_x) * dim_vy
        u = np.asfortranarray((lb_vx * np.ones((self.nx, self.ny))).astype(np.float32))
        v = np.asfortranarray((lb_vy * np.ones((self.nx, self.ny))).astype(np.float32))
        self.sim.set_fields(rho, u, v)

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb; None = exactly feq."""
        self.sim.init_pop(perturb)
