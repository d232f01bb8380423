"""A D2Q9 relaxation solver for a Poisson problem in a box: the surface of the reference's ``LB_D2Q9.poisson.solver``
(``Poisson_Solver``) on a Poisson handle of liblbhip (``Simulation(..., semantics='poisson', bc='dirichlet')``).

``rho`` relaxes towards the solution of ``laplace(rho) = -source`` (up to the scheme's factors) with ``rho_on_boundary``
prescribed on the four walls.  ``run(n)`` is the reference's loop -- iterate, and from the second iteration since the last
``update_source`` stop as soon as ``mean |rho - rho_before| / mean rho_before < tolerance`` -- but where the reference makes
six launches, six host waits, two reductions and two read-backs per iteration, here an iteration is one fused launch plus
one small one, the decision is taken on the device, and the host looks at four bytes once per batch of iterations.  The
state a stopped run leaves is exactly the one after the iteration that met the rule.  The phase methods run one kernel each.

Restated as the reference has it: the source is scaled by ``lb_D delta_t`` on the host AND multiplied by
``delta_t lb_D`` in the collision; ``update_negative_gradient`` stores MINUS the y-difference in ``u`` and MINUS the
x-difference in ``v``.  Differences: ``converged`` replaces the reference's ``print``; ``init_pop`` takes a ``seed`` (the
reference draws an unseeded perturbation -- of a lattice that is zero); the OpenCL-only arguments are accepted and ignored.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, DropIn, cs, get_divisible_global, lattice_arrays  # noqa: F401
from ..simulation import Simulation

w, cx, cy = lattice_arrays(np.float32, np.int32)


# ---- parameter arithmetic: no handle, no GPU -----------------------------------------------------------------------
def poisson_parameters(delta_t, delta_x):
    """solver.py:79-83, 143-150: delta_x, delta_t float32; lb_D = float32(delta_t / delta_x^2); omega = float32 of the
    float64 expression 1 / (0.5 + lb_D / cs^2); source_scale = lb_D delta_t, what update_source multiplies the source
    by; react_factor = delta_t lb_D, what collide_particles multiplies it by once more."""
    delta_x, delta_t = np.float32(delta_x), np.float32(delta_t)
    lb_D = np.float32(delta_t / delta_x ** 2)
    omega = np.float32((.5 + float(lb_D) / cs ** 2) ** -1.)
    assert omega < 2.
    return dict(delta_x=delta_x, delta_t=delta_t, ulb=delta_t / delta_x, lb_D=lb_D, omega=omega,
                source_scale=np.float32(lb_D * delta_t), react_factor=np.float32(delta_t * lb_D))


class Poisson_Solver(DropIn):
    _sim = property(lambda self: self.sim)      # the engine under the name the shared methods use

    def __init__(self, nx=None, ny=None, sources=None, delta_t=None, delta_x=None, rho_on_boundary=0.0,
                 tolerance=10. ** -6., context=None, queue=None,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False, device=0, seed=None):
        self.nx, self.ny = np.int32(nx), np.int32(ny)
        self.input_sources = sources
        self.scaled_sources = None
        self.use_interop = use_interop
        self.rho_on_boundary = np.float32(rho_on_boundary)
        self.tolerance = np.float32(tolerance)

        p = poisson_parameters(delta_t, delta_x)
        self.delta_x, self.delta_t, self.ulb = p["delta_x"], p["delta_t"], p["ulb"]
        print('u_lb:', self.ulb)
        self.lb_D, self.omega = p["lb_D"], p["omega"]
        print('omega', self.omega)

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)
        self.context, self.queue = context, queue       # (OpenCL objects of the reference: kept, never used)

        self.sim = Simulation(int(nx), int(ny), self.omega, bc="dirichlet", semantics="poisson", device=device)
        self.sim.set_poisson(self.rho_on_boundary, p["react_factor"], self.tolerance)
        self.converged = False
        self._seed = seed
        # rho = 0, u = v = 0 (init_hydro), feq from it, f = feq x noise: all zero, like the handle's fresh state
        self._uv = {"u": np.zeros((int(nx), int(ny)), np.float32, order='F'), "v": np.zeros((int(nx), int(ny)), np.float32, order='F')}
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")
        self.update_source(sources)
        self.update_feq()
        self.init_pop()

    sources = property(lambda self: self.input_sources)
    num_iterations = property(lambda self: self.sim.solve_state()[0])

    def _read_field(self, key):
        if key in self._uv:
            return self._uv[key].copy(order='F')
        return self.sim.get_fields((key,))[key]

    def set_D_and_omega(self):
        p = poisson_parameters(self.delta_t, self.delta_x)
        self.lb_D, self.omega = p["lb_D"], p["omega"]

    def update_source(self, new_source):
        """Pass in a new source -- an (nx, ny) numpy array, or a float32 torch tensor on the device, which never visits the
        host.  Restarts the iteration count with the old density as the first guess."""
        self.input_sources = new_source
        scale = np.float32(self.lb_D * self.delta_t)
        if hasattr(new_source, "data_ptr"):
            self.scaled_sources = new_source * float(scale)
        else:
            self.scaled_sources = np.asfortranarray(np.array(new_source, dtype=np.float32) * scale)
        self.sim.set_source(self.scaled_sources)
        self.sim.solve_reset()
        self.converged = False

    def update_negative_gradient(self):
        """u = -(d rho / dy), v = -(d rho / dx): the reference's names (D2Q9_poisson.cl:300-301)."""
        ddx, ddy = self.sim.gradient(float(self.delta_x))
        self._uv = {"u": -ddy, "v": -ddx}

    def init_pop(self, amplitude=10. ** -5., seed=None):
        """f = f_streamed = feq (1 + amplitude randn), seeded."""
        rng = np.random.default_rng(self._seed if seed is None else seed)
        self.sim.init_pop(1. + amplitude * rng.standard_normal((int(self.nx), int(self.ny), NUM_JUMPERS)))

    def run(self, num_iterations):
        """Up to num_iterations iterations; stops by the reference's rule, then sets `converged` and updates u, v."""
        _, converged, _ = self.sim.solve(num_iterations)
        if converged:
            self.converged = True
            self.update_negative_gradient()

    def get_fields(self):
        return self.sim.get_fields(("f", "rho", "feq"))
