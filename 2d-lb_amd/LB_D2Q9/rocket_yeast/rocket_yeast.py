"""A growing colony propelled by the surfactant it secretes: the surface of the reference's
``LB_D2Q9.rocket_yeast.rocket_yeast`` (class ``Rocket_Yeast``) on a pair of rocket handles of liblbhip
(``LB_D2Q9.coupled.Surfactant_Colony(..., mode='flow')``).

Two scalar lattices in a periodic box, the population (index 0) and the surfactant (index 1).  The velocity that advects both
is ``-epsilon / cs^2`` times the D2Q9 stencil over the surfactant (a Marangoni flow); the population grows logistically, feels
the Shan-Chen self-attraction ``-G_chen psi grad psi`` and secretes surfactant at the rate ``Gc``.  ``run(n)`` is the reference's
loop -- move, update_hydro (with update_u_and_v and update_force), update_feq, collide_particles -- but where the reference makes
nine launches, nine host waits and a full copy of ``f`` per step, here a step is one fused launch.  The phase methods run one
stage each and are bitwise equal to it.

The constants (``omega``, ``omega_c``, ``lb_G``, ``lb_Gc``, ``nx``, ``ny`` ...) are derived in the reference's order and precision:
under the numpy the reference was written for, a float32 scalar combined with a Python number is a float64, so every expression
is float64 up to the ``np.float32(...)`` the reference writes.  Differences: ``psi`` and the pseudo-force are ``(nx, ny)`` (the
reference allocates ``(ny, ny)``, which its kernels overrun when nx > ny); the noisy droplet is drawn from
``np.random.default_rng(rng)`` (the reference draws unseeded); ``check_max_ulb`` checks once per ``run()`` call, not after every
kernel; ``two_d_local_size`` and ``use_interop`` are accepted and ignored; nothing is printed unless ``verbose=True``.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, Phases, get_divisible_global, lattice_arrays, w0, w1, w2  # noqa: F401
from ..coupled import Surfactant_Colony

w, cx, cy = lattice_arrays(np.float32, np.int32)
cs = np.float32(1. / np.sqrt(3))                # Speed of sound on the lattice


class Rocket_Yeast(Phases):
    """Everything is in dimensionless units.  It's just easier."""
    _MODE = "flow"
    _KEYS = ("rho", "f", "feq", "u", "v", "psi", "pseudo_force_x", "pseudo_force_y")

    def __init__(self, Lx=1.0, Ly=1.0, R0=5., epsilon=1., Dc=1. / 4., Gc=2.0, rho_o=1.0, G_chen=-1.0, time_prefactor=1., N=10,
                 two_d_local_size=(32, 32), use_interop=False, check_max_ulb=False, mach_tolerance=0.1, rng=None, device=0,
                 verbose=False, **extra):
        self.verbose = verbose
        self.Lx, self.Ly = Lx, Ly
        self.D, self.G = 1. / 4., 1.
        self.Dc = (1. / 4.) * np.float64(np.float32(Dc))
        self.Gc = np.float32(Gc)
        self.epsilon = np.float32(epsilon)
        self.R0 = R0
        self.rho_o, self.G_chen = np.float32(rho_o), np.float32(G_chen)
        self._more_parameters(**extra)
        self.num_populations, self.pop_index, self.surf_index = np.int32(2), np.int32(0), np.int32(1)
        self.use_interop, self.check_max_ulb, self.mach_tolerance = use_interop, check_max_ulb, mach_tolerance
        self.L = self.T = 1.0
        self.N = N
        self.delta_x, self.delta_t = self._discretization(N, time_prefactor)
        self.ulb = self.delta_t / self.delta_x
        self._say('u_lb:', self.ulb)
        cs2 = np.float64(cs) ** 2                       # (cs ** 2: a float32 scalar and a Python int)
        ratio = np.float64(self.delta_t) / np.float64(self.delta_x) ** 2
        self.lb_D = np.float32(self.D * ratio)
        self.omega = np.float32((.5 + np.float64(self.lb_D) / cs2) ** -1.)
        self._say('omega', self.omega)
        assert self.omega < 2.
        self.lb_G = np.float32(self.G * np.float64(self.delta_t))
        self.lb_Dc = np.float32(self.Dc * ratio)
        self.omega_c = np.float32((.5 + np.float64(self.lb_Dc) / cs2) ** -1.)
        self._say('omega_s', self.omega_c)
        assert self.omega_c < 2.
        self.lb_Gc = np.float32(np.float64(self.Gc) * np.float64(self.delta_t))
        self.nx = self.ny = None
        self.initialize_grid_dims()
        self.two_d_local_size = two_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.context = self.queue = self.kernels = None     # (OpenCL objects of the reference: kept, never used)
        self.w, self.cx, self.cy = w, cx, cy
        self.halo = np.int32(1)
        self.buf_nx, self.buf_ny = np.int32(two_d_local_size[0] + 2), np.int32(two_d_local_size[1] + 2)
        self.psi_local = None
        self._rng = np.random.default_rng(rng)
        self._sim = self._engine = Surfactant_Colony(int(self.nx), int(self.ny), self.omega, self.omega_c, mode=self._MODE, device=device)
        self._engine.set_params(**self._engine_params())
        for key in self._KEYS:
            setattr(self, key, DeviceField(self, key))
        self.f_streamed = self.f
        self.init_hydro()
        self.update_feq()
        self.init_pop()

    # -- what the two classes derive differently ---------------------------------------------------------------------------
    def _more_parameters(self):
        pass

    def _discretization(self, N, time_prefactor):
        delta_x = 1. / N
        return delta_x, time_prefactor * delta_x ** 2

    def _engine_params(self):
        return dict(G=self.lb_G, G_c=self.lb_Gc, epsilon=self.epsilon, rho_o=self.rho_o, G_chen=self.G_chen)

    # -- plumbing ------------------------------------------------------------------------------------------------------------
    def _say(self, *args):
        if self.verbose:
            print(*args)

    @property
    def engine(self):
        """The ``Surfactant_Colony`` underneath (set_f, set_variant, checkpoints, hot_kernel ...)."""
        return self._engine

    def _read_field(self, key):
        return self._engine.get_fields((key,))[key]

    def initialize_grid_dims(self):
        self.nx = np.int32(np.round(self.N * self.Lx))
        self.ny = np.int32(np.round(self.N * self.Ly))
        self._say('nx:', self.nx)
        self._say('ny:', self.ny)

    def init_hydro(self):
        """The noisy Gaussian droplet, no surfactant; then the velocity and the forces it implies."""
        nx, ny = int(self.nx), int(self.ny)
        self.x_center, self.y_center = nx // 2, ny // 2
        Y, X = np.meshgrid(np.arange(ny), np.arange(nx))
        self.X = (X.astype(np.float64) - self.x_center) / self.N
        self.Y = (Y.astype(np.float64) - self.y_center) / self.N
        rho_host = np.zeros((nx, ny, 2), dtype=np.float32, order='F')
        rho_host[:, :, self.pop_index] = 1.0 * np.exp(-(self.X ** 2 + self.Y ** 2) / self.R0 ** 2) * (1 + .05 * self._rng.standard_normal((nx, ny)))
        rho_host[:, :, self.surf_index] = 0.0
        zero = np.zeros((nx, ny), np.float32)
        self._engine.set_fields(rho_host, zero, zero)
        self._stage_three()

    def _stage_three(self):
        self.update_u_and_v()
        self.update_force()

    def redo_initial_condition(self, rho_field):
        """After you have specified your own IC: rho_field (nx, ny, 2)."""
        g = self._engine.get_fields(("u", "v"))
        self._engine.set_fields(np.asarray(rho_field, dtype=np.float32), g["u"], g["v"])
        self._stage_three()
        self.update_feq()
        self.init_pop()

    def init_pop(self, amplitude=0):
        """f = f_streamed = feq (1 + amplitude randn), from the class's generator; amplitude 0 = exactly feq."""
        if amplitude == 0:
            self._engine.init_pop(None)
        else:
            self._engine.init_pop(1. + amplitude * self._rng.standard_normal((int(self.nx), int(self.ny), 2, NUM_JUMPERS)))

    def move_bcs(self):
        pass                                            # (implemented in move_periodic, as in the reference)

    def _warn_max_ulb(self):
        g = self._engine.get_fields(("u", "v"))
        max_ulb = float(np.sqrt(g["u"].astype(np.float64) ** 2 + g["v"].astype(np.float64) ** 2).max())
        if max_ulb > cs * self.mach_tolerance:
            print('max_ulb is greater than cs/10! Ma=', max_ulb / cs)

    def update_u_and_v(self):
        self._engine.update_velocity()

    def update_hydro(self):
        self._engine.update_hydro()
        self._stage_three()

    def update_force(self):
        self._engine.update_forces()

    def run(self, num_iterations):
        """num_iterations time steps, one fused launch each."""
        self._engine.run(int(num_iterations))
        if self.check_max_ulb:
            self._warn_max_ulb()

    def get_fields(self):
        return {k: self._read_field(k) for k in self._KEYS}
