"""A colony that eats a nutrient and pushes itself outwards: the surface of the reference's
``LB_D2Q9.reaction_diffusion.surfactant_nutrient_waves`` (``Surfactant_Nutrient_Wave``, ``Clumpy_Surfactant_Nutrient_Wave``) on two
scalar-lattice handles of liblbhip and an ``lb_spectral`` (``LB_D2Q9.nutrient_set.Nutrient_Set``).

Two scalar lattices in a periodic box, the population (index 0, ``omega``) and the nutrient (index 1, ``omega_n``).  Every step
solves ``(1 - lam^2 laplace) phi = rho_p`` and sets ``(u, v) = -vc (delta_t / delta_x) Re grad phi`` for both; the population grows
by ``w_k G rho_p rho_n`` and the nutrient is depleted by the same amount; the clumpy class adds the Shan-Chen self-attraction of the
population.  ``run(n)`` is fused HIP -- five launches per step, no host wait (lb_run_nutrient) -- where the reference makes some 25
launches and array passes and waits after each; the phase methods run the reference's sequence un-fused.

Everything is in dimensionless units: ``L = T = 1``, ``D = 1/4``, ``G = 1``.  The parameter arithmetic lives in
``surfactant_nutrient_parameters`` and needs no handle: it is the reference's, float64 up to the ``np.float32(...)`` the reference
writes.  Repairs: Python 2 prints (nothing is printed unless ``verbose=True``); ``np.float``; ``nx / 2`` is
``nx // 2``; the droplet is laid out with ``indexing='ij'``; ``cl_context`` / ``cl_queue`` are gone; ``psi`` and the pseudo-force are
``(nx, ny)`` (the reference allocates ``(ny, ny)``); the 5 % noise of ``init_hydro`` and the perturbation of ``init_pop`` are drawn
from ``np.random.default_rng(rng)``; ``check_max_ulb`` goes through the engine's health check, once per call.  Grid sizes must be
``2^a 3^b 5^c <= 4096`` on each axis (the transform's lengths): anything else raises ``LbError`` before a device is touched.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, Phases, get_divisible_global, lattice_arrays, w0, w1, w2  # noqa: F401
from ..nutrient_set import Nutrient_Set

w, cx, cy = lattice_arrays(np.float32, np.int32)
cs = np.float32(1. / np.sqrt(3))                # Speed of sound on the lattice


# ---- parameter arithmetic: no handle, no GPU -----------------------------------------------------------------------
def surfactant_nutrient_parameters(Lx=1.0, Ly=1.0, vc=1., lam=1., Dn=1. / 4., R0=5., time_prefactor=1., N=50):
    """delta_x = 1 / N, delta_t = time_prefactor delta_x^2; D = 1/4, Dn and G = 1 in lattice units, both relaxation rates, the grid
    (round(N Lx), round(N Ly)) and the factor between Re grad phi and the lattice velocity."""
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    cs2 = np.float64(cs) ** 2                   # (cs ** 2: a float32 scalar and a Python int)
    ratio = delta_t / delta_x ** 2
    lb_D = np.float32(.25 * ratio)
    omega = np.float32((.5 + np.float64(lb_D) / cs2) ** -1.)
    assert omega < 2.
    lb_Dn = np.float32(Dn * ratio)
    omega_n = np.float32((.5 + np.float64(lb_Dn) / cs2) ** -1.)
    assert omega_n < 2.
    return dict(N=N, delta_x=delta_x, delta_t=delta_t, ulb=delta_t / delta_x, D=.25, Dn=Dn, G=1., vc=vc, lam=lam, R0=R0,
                lb_D=lb_D, omega=omega, lb_Dn=lb_Dn, omega_n=omega_n, lb_G=np.float32(1. * delta_t),
                nx=int(np.round(N * Lx)), ny=int(np.round(N * Ly)), scale=-vc * (delta_t / delta_x))


class Surfactant_Nutrient_Wave(Phases):
    """Everything is in dimensionless units.  It's just easier."""
    _KEYS = ("rho", "f", "feq", "u", "v")

    def __init__(self, Lx=1.0, Ly=1.0, vc=1., lam=1., Dn=1. / 4., R0=5., time_prefactor=1., N=50,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False,
                 check_max_ulb=False, mach_tolerance=0.1, device=0, rng=None, verbose=False):
        self.verbose = verbose
        self.Lx, self.Ly = Lx, Ly
        self.D, self.Dn, self.G = 1. / 4., Dn, 1.
        self.vc, self.lam, self.R0 = vc, lam, R0
        self.num_populations, self.pop_index, self.nut_index = np.int32(2), np.int32(0), np.int32(1)
        self.use_interop, self.check_max_ulb, self.mach_tolerance = use_interop, check_max_ulb, mach_tolerance
        self.L = self.T = 1.0

        p = surfactant_nutrient_parameters(Lx=Lx, Ly=Ly, vc=vc, lam=lam, Dn=Dn, R0=R0, time_prefactor=time_prefactor, N=N)
        self.N, self.delta_x, self.delta_t, self.ulb = p["N"], p["delta_x"], p["delta_t"], p["ulb"]
        self._say('u_lb:', self.ulb)
        self.lb_D, self.omega, self.lb_Dn, self.omega_n, self.lb_G = p["lb_D"], p["omega"], p["lb_Dn"], p["omega_n"], p["lb_G"]
        self._say('omega', self.omega)
        self._say('omega_n', self.omega_n)
        self.nx, self.ny = np.int32(p["nx"]), np.int32(p["ny"])
        self._say('nx:', self.nx)
        self._say('ny:', self.ny)
        self.velocity_scale = np.float32(p["scale"])

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)
        self.context = self.queue = self.kernels = None     # (OpenCL objects of the reference: kept, never used)
        self.w, self.cx, self.cy = w, cx, cy

        self._rng = np.random.default_rng(rng)
        self._sim = self._engine = Nutrient_Set(int(self.nx), int(self.ny), self.omega, self.omega_n, lam=lam, dx=self.delta_x, device=device)
        self._engine.set_params(**self._engine_params())
        self.poisson_solver = self._engine.solver
        for key in self._KEYS:
            setattr(self, key, DeviceField(self, key))
        self.f_streamed = self.f
        self.x_center = self.y_center = self.X = self.Y = None
        self.init_hydro()
        self.update_feq()
        self.init_pop()

    def _engine_params(self):
        return dict(G=self.lb_G, scale=self.velocity_scale, clumpy=False)

    # -- plumbing ------------------------------------------------------------------------------------------------------------
    def _say(self, *args):
        if self.verbose:
            print(*args)

    @property
    def engine(self):
        """The ``Nutrient_Set`` underneath (set_f, use_stream, the members' checkpoints ...)."""
        return self._engine

    def _read_field(self, key):
        return self._engine.get_fields((key,))[key]

    def initialize_grid_dims(self):
        self.nx = np.int32(np.round(self.N * self.Lx))
        self.ny = np.int32(np.round(self.N * self.Ly))

    # -- state -----------------------------------------------------------------------------------------------------------------
    def init_hydro(self):
        """The noisy Gaussian droplet on a uniform nutrient; then the velocity (and the force) it implies."""
        nx, ny = int(self.nx), int(self.ny)
        self.x_center, self.y_center = nx // 2, ny // 2
        X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
        self.X = (X.astype(np.float64) - self.x_center) / self.N
        self.Y = (Y.astype(np.float64) - self.y_center) / self.N
        rho_host = np.zeros((nx, ny, 2), dtype=np.float32, order='F')
        rho_host[:, :, self.pop_index] = 1.2 * np.exp(-(self.X ** 2 + self.Y ** 2) / self.R0 ** 2) * (1 + .05 * self._rng.standard_normal((nx, ny)))
        rho_host[:, :, self.nut_index] = 1.0
        zero = np.zeros((nx, ny), np.float32)
        self._engine.set_fields(rho_host, zero, zero)
        self._stage_three()

    def _stage_three(self):
        self.update_u_and_v()

    def redo_initial_condition(self, rho_field):
        """After you have specified your own IC: rho_field (nx, ny, 2)."""
        zero = np.zeros((int(self.nx), int(self.ny)), np.float32)
        self._engine.set_fields(np.asarray(rho_field, dtype=np.float32), zero, zero)
        self._stage_three()
        self.update_feq()
        self.init_pop()

    def init_pop(self, amplitude=0):
        """f = f_streamed = feq (1 + amplitude randn), from the class's generator; amplitude 0 = exactly feq."""
        if amplitude == 0:
            self._engine.init_pop(None)
        else:
            self._engine.init_pop(1. + amplitude * self._rng.standard_normal((int(self.nx), int(self.ny), 2, NUM_JUMPERS)))

    def _check_ulb(self):
        if self.check_max_ulb:
            mach = self._engine.members[0].check()["max_mach"]
            if mach > self.mach_tolerance:
                print('max_ulb is greater than cs/10! Ma=', mach)

    # -- the phases (move, update_feq: Phases) -----------------------------------------------------------------------------------
    def move_bcs(self):
        pass                                            # (implemented in move_periodic, as in the reference)

    def update_u_and_v(self):
        """(u, v) = -vc (delta_t / delta_x) Re grad phi of the stored rho_p, for both lattices (lb_nutrient_velocity)."""
        self._engine.update_velocity()
        self._check_ulb()

    def update_hydro(self):
        self._engine.update_hydro()
        self._stage_three()

    def update_force(self):
        pass                                            # (the clumpy class has one)

    def run(self, num_iterations):
        """num_iterations time steps, fused on the device; returns with the work complete."""
        self._engine.run(int(num_iterations))
        self._check_ulb()

    def get_fields(self):
        return {k: self._read_field(k) for k in self._KEYS}


class Clumpy_Surfactant_Nutrient_Wave(Surfactant_Nutrient_Wave):
    _KEYS = Surfactant_Nutrient_Wave._KEYS + ("psi", "pseudo_force_x", "pseudo_force_y")

    def __init__(self, rho_o=1.0, G_chen=-1.0, **kwargs):
        self.rho_o, self.G_chen = np.float32(rho_o), np.float32(G_chen)
        self.halo = np.int32(1)
        local = kwargs.get("two_d_local_size", (32, 32))
        self.buf_nx, self.buf_ny = np.int32(local[0] + 2), np.int32(local[1] + 2)
        self.psi_local = None
        super(Clumpy_Surfactant_Nutrient_Wave, self).__init__(**kwargs)

    def _engine_params(self):
        return dict(G=self.lb_G, scale=self.velocity_scale, clumpy=True, rho_o=self.rho_o, G_chen=self.G_chen)

    def _stage_three(self):
        self.update_u_and_v()
        self.update_force()

    def update_force(self):
        """psi of the stored rho_p and the pseudo-force F = -cs^2 G_chen psi grad_w psi (lb_update_forces_nutrient)."""
        self._engine.update_forces()
