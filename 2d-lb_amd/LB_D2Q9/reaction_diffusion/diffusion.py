"""Scalar transport on the D2Q9 lattice: the surface of the reference's ``LB_D2Q9.reaction_diffusion.diffusion``
(``Diffusion``, ``Advection_Diffusion``, ``Reaction_Diffusion``, ``Reaction_Advection_Diffusion``) on a scalar-lattice
handle of liblbhip (``Simulation(..., semantics='diffusion', bc='open')``).

A concentration ``rho`` is carried by nine populations with the linear equilibrium ``w_k rho (1 + 3 c_k.u)``; ``u, v``
are imposed, never computed; the two Fisher classes add ``w_k G rho (1 - rho)`` in the collision.  ``run(n)`` is fused
HIP (one launch per step where the reference makes five and waits after each); the phase methods run one kernel each.

The parameter arithmetic lives in plain functions (``diffusion_parameters`` ...) that need no handle.  Restated as the
reference has it, with three repairs: ``np.float`` no longer exists; the Gaussian of ``init_hydro`` is
laid out with ``indexing='ij'`` so that it also fits boxes that are not square (identical where the reference runs);
the Fisher collision gets its arguments in the kernel's order.  ``init_pop(perturb=None)`` takes the perturbation as an
argument (the reference draws an unseeded one of amplitude 0.001).  ``Reaction_Advection_Diffusion_Stochastic`` is not
offered: it launches a kernel the reference's .cl file does not contain.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, DropIn, cs, get_divisible_global, lattice_arrays  # noqa: F401
from ..simulation import Simulation

w, cx, cy = lattice_arrays(np.float32, np.int32)


# ---- parameter arithmetic: no handle, no GPU -----------------------------------------------------------------------
def lattice_discretisation(N, time_prefactor):
    """delta_x = 1 / N, delta_t = time_prefactor delta_x^2, u_lb = delta_t / delta_x."""
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    return dict(N=N, delta_x=delta_x, delta_t=delta_t, ulb=delta_t / delta_x)


def omega_of(lb_D):
    omega = (.5 + lb_D / cs ** 2) ** -1.
    assert omega < 2.
    return omega


def grid_dims(Lx, Ly, L, N):
    lx, ly = N * int(Lx / L), N * int(Ly / L)
    return dict(lx=lx, ly=ly, nx=lx + 2, ny=ly + 2)


def diffusion_parameters(Lx=1.0, Ly=1.0, D=1.0, z=0.1, time_prefactor=1., N=50):
    """Diffusion: L = z, T = z^2 / D, lattice diffusivity delta_t / delta_x^2."""
    p = dict(L=z, T=z ** 2 / D)
    p.update(lattice_discretisation(N, time_prefactor))
    p["lb_D"] = p["delta_t"] / p["delta_x"] ** 2
    p["omega"] = omega_of(p["lb_D"])
    p.update(grid_dims(Lx, Ly, p["L"], N))
    return p


def advection_diffusion_parameters(vx=1.0, vy=1.0, vc=1.0, Lx=1.0, Ly=1.0, D=1.0, z=0.1, time_prefactor=1., N=50):
    """Advection_Diffusion: L = z, T = z / vc, Pe = z vc / D, lattice diffusivity (delta_t / delta_x^2) / Pe; the uniform
    imposed velocity in lattice units is (delta_t / delta_x) (vx, vy) / vc."""
    p = dict(L=z, T=z / vc)
    p.update(lattice_discretisation(N, time_prefactor))
    p["Pe"] = z * vc / D
    p["lb_D"] = (p["delta_t"] / p["delta_x"] ** 2) * (1. / p["Pe"])
    p["omega"] = omega_of(p["lb_D"])
    p.update(grid_dims(Lx, Ly, p["L"], N))
    p["lb_vx"] = (p["delta_t"] / p["delta_x"]) * (vx / vc)
    p["lb_vy"] = (p["delta_t"] / p["delta_x"]) * (vy / vc)
    return p


def reaction_diffusion_parameters(g=1.0, **kwargs):
    """Reaction_Diffusion: Diffusion's scales; G_dim = T g, G = G_dim delta_t."""
    p = diffusion_parameters(**kwargs)
    p["G_dim"] = p["T"] * g
    p["G"] = p["G_dim"] * p["delta_t"]
    return p


def reaction_advection_diffusion_parameters(g=1.0, **kwargs):
    """Reaction_Advection_Diffusion: Advection_Diffusion's scales; G as above; Fisher speed 2 sqrt(G_dim / Pe)."""
    p = advection_diffusion_parameters(**kwargs)
    p["G_dim"] = p["T"] * g
    p["G"] = p["G_dim"] * p["delta_t"]
    p["vf_dim"] = 2 * np.sqrt((1. / p["Pe"]) * p["G_dim"])
    return p


def gaussian_blob(nx, ny, N):
    """rho = exp(-(X^2 + Y^2)) around the box centre, X, Y in units of the characteristic length; (nx, ny) arrays."""
    x_center, y_center = nx // 2, ny // 2
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    X_dim = (X.astype(np.float64) - x_center) / N
    Y_dim = (Y.astype(np.float64) - y_center) / N
    rho = np.asfortranarray(np.exp(-(X_dim ** 2 + Y_dim ** 2)).astype(np.float32))
    return x_center, y_center, X_dim, Y_dim, rho


class Diffusion(DropIn):
    """A Gaussian blob of concentration diffusing in a box (the reference's verification case)."""

    _bc = "open"       # the reference's box: move_bcs does nothing
    _sim = property(lambda self: self.sim)      # the engine under the name the shared methods use

    def __init__(self, Lx=1.0, Ly=1.0, D=1.0, z=0.1, time_prefactor=1., N=50,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False, device=0):
        self.phys_Lx, self.phys_Ly, self.phys_D, self.phys_z = Lx, Ly, D, z
        self.use_interop = use_interop
        self.time_prefactor = time_prefactor
        self.L = self.T = None
        self.set_characteristic_length_time()
        print('Characteristic L:', self.L)
        print('Characteristic T:', self.T)

        d = lattice_discretisation(N, time_prefactor)
        self.N, self.delta_x, self.delta_t, self.ulb = d["N"], d["delta_x"], d["delta_t"], d["ulb"]
        print('u_lb:', self.ulb)

        self.lb_D = self.omega = None
        self.set_D_and_omega()

        self.lx = self.ly = self.nx = self.ny = None
        self.initialize_grid_dims()

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)
        print('2d global:', self.two_d_global_size)
        print('2d local:', self.two_d_local_size)
        print('3d global:', self.three_d_global_size)
        print('3d local:', self.three_d_local_size)

        self.sim = Simulation(self.nx, self.ny, self.omega, bc=self._bc, semantics="diffusion", device=device)
        self.sim.set_reaction(getattr(self, "G", None) or 0.)
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")

        self.x_center = self.y_center = self.X_dim = self.Y_dim = None
        self.init_hydro()
        self.update_feq()
        self.init_pop()

    # -- parameters (overridden by the subclasses as in the reference) ---------------------------------------------------
    def set_characteristic_length_time(self):
        self.L = self.phys_z
        self.T = self.phys_z ** 2 / self.phys_D

    def set_D_and_omega(self):
        self.lb_D = self.delta_t / self.delta_x ** 2
        self.omega = omega_of(self.lb_D)
        print('omega', self.omega)

    def initialize_grid_dims(self):
        g = grid_dims(self.phys_Lx, self.phys_Ly, self.L, self.N)
        self.lx, self.ly, self.nx, self.ny = g["lx"], g["ly"], g["nx"], g["ny"]

    # -- state -----------------------------------------------------------------------------------------------------------
    def _imposed_velocity(self):
        z = np.zeros((self.nx, self.ny), dtype=np.float32, order='F')
        return z, z.copy(order='F')

    def init_hydro(self):
        self.x_center, self.y_center, self.X_dim, self.Y_dim, rho = gaussian_blob(self.nx, self.ny, self.N)
        u, v = self._imposed_velocity()
        self.sim.set_fields(rho, u, v)

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb; None = exactly feq.  (The reference multiplies by 1 + 0.001 randn, unseeded.)"""
        self.sim.init_pop(perturb)


class Advection_Diffusion(Diffusion):
    def __init__(self, vx=1.0, vy=1.0, vc=1.0, **kwargs):
        self.phys_vx, self.phys_vy, self.phys_vc = vx, vy, vc
        self.Pe = None
        super(Advection_Diffusion, self).__init__(**kwargs)

    def set_characteristic_length_time(self):
        self.L = self.phys_z
        self.T = self.phys_z / self.phys_vc

    def set_D_and_omega(self):
        self.Pe = self.phys_z * self.phys_vc / self.phys_D
        print('Pe:', self.Pe)
        self.lb_D = (self.delta_t / self.delta_x ** 2) * (1. / self.Pe)
        self.omega = omega_of(self.lb_D)
        print('omega', self.omega)

    def _imposed_velocity(self):
        lb_vx = (self.delta_t / self.delta_x) * (self.phys_vx / self.phys_vc)
        lb_vy = (self.delta_t / self.delta_x) * (self.phys_vy / self.phys_vc)
        u = np.asfortranarray((lb_vx * np.ones((self.nx, self.ny))).astype(np.float32))
        v = np.asfortranarray((lb_vy * np.ones((self.nx, self.ny))).astype(np.float32))
        return u, v


class Reaction_Diffusion(Diffusion):
    """Fisher waves: diffusion plus logistic growth."""

    def __init__(self, g=1.0, **kwargs):
        self.g = g
        self.G_dim = self.G = None
        super(Reaction_Diffusion, self).__init__(**kwargs)

    def set_D_and_omega(self):
        self.G_dim = self.T * self.g
        print('Gd_dim:', self.G_dim)
        self.G = self.G_dim * self.delta_t
        print('G_lb:', self.G)
        self.lb_D = 1.0 * (self.delta_t / self.delta_x ** 2)
        self.omega = omega_of(self.lb_D)
        print('omega', self.omega)


class Reaction_Advection_Diffusion(Advection_Diffusion):
    def __init__(self, g=1.0, **kwargs):
        self.g = g
        self.G_dim = self.G = None
        self.vf_dim = None
        super(Reaction_Advection_Diffusion, self).__init__(**kwargs)

    def set_D_and_omega(self):
        super(Reaction_Advection_Diffusion, self).set_D_and_omega()
        self.G_dim = self.T * self.g
        print('Gd_dim:', self.G_dim)
        self.G = self.G_dim * self.delta_t
        print('G_lb:', self.G)
        self.vf_dim = 2 * np.sqrt((1. / self.Pe) * self.G_dim)
        print('Dimensionless Fisher Wave Velocity:', self.vf_dim)
