"""What the drop-in class families share (``dimensionless.hip_dim``, ``dimensionless.cython_dim``,
``reaction_diffusion.diffusion``): the lattice constants, the ``cl.Buffer`` stand-in, the methods that only forward to
the engine, and the pipe classes' grid and density-ramp arithmetic.  Internal: import the names from those modules."""
import numpy as np

from .masks import disc_pixels

# ---- D2Q9 lattice constants (opencl_dim.py:22-36, cython_dim.pyx:16-29) ----------------------------------------------
NUM_JUMPERS = 9
cs = 1. / np.sqrt(3)
cs2 = cs ** 2
cs22 = 2 * cs2
cssq = 2.0 / 9.0
two_cs4 = 2 * cs ** 4
w0, w1, w2 = 4. / 9., 1. / 9., 1. / 36.


def lattice_arrays(float_dtype=None, int_dtype=None):
    """(w, cx, cy); the OpenCL-side modules export them as float32 / int32, the Cython-side one with numpy's defaults."""
    return (np.array([w0] + 4 * [w1] + 4 * [w2], dtype=float_dtype),
            np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=int_dtype),
            np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=int_dtype))


def get_divisible_global(global_size, local_size):
    """Smallest multiple of local_size that covers global_size, per dimension (opencl_dim.py:39-56; kept for the
    attributes the reference's classes show: the HIP launches do not use it)."""
    return tuple(-(-g // l) * l for g, l in zip(global_size, local_size))


class DeviceField(object):
    """Stand-in for the reference's ``cl.Buffer`` / live-array attributes (``sim.rho``, ``sim.f`` ...): a named view of
    the owner's engine state; ``.get()`` or ``np.asarray(...)`` give a host copy."""

    def __init__(self, owner, key):
        self._owner, self._key = owner, key

    def get(self):
        return self._owner._read_field(self._key)

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a if dtype is None else a.astype(dtype)


class Phases(object):
    """The reference's five phase methods, forwarded to the engine (``self._sim``: a ``Simulation`` or a set of them)."""

    def move_bcs(self):
        self._sim.move_bcs()

    def move(self):
        self._sim.move()

    def update_hydro(self):
        self._sim.update_hydro()

    def update_feq(self):
        self._sim.update_feq()

    def collide_particles(self):
        self._sim.collide_particles()


class DropIn(Phases):
    """The other methods of a drop-in class that only forward to its engine."""

    def _say(self, *args):
        if self.verbose:
            print(*args)

    def _read_field(self, key):
        return self._sim.get_fields((key,))[key]

    def run(self, num_iterations):
        """num_iterations time steps, fused on the device (one phase method = one un-fused kernel)."""
        self._sim.run(num_iterations)

    def step(self):
        self._sim.run(1)

    def get_fields(self):
        return self._sim.get_fields()

    def get_nondim_fields(self):
        fields = self.get_fields()
        fields['u'] *= self.delta_x / self.delta_t
        fields['v'] *= self.delta_x / self.delta_t
        return fields

    def get_physical_fields(self):
        fields = self.get_nondim_fields()
        fields['u'] *= (self.L / self.T)
        fields['v'] *= (self.L / self.T)
        return fields


class PipeDropIn(DropIn):
    """Grid and initial state the OpenCL-side and the Cython-side pipe classes derive alike."""

    def initialize_grid_dims(self):
        """lx = ceil(pipe_length / L * N), ly = N; one boundary node more in each direction (opencl_dim.py:191-201)."""
        self.lx = int(np.ceil((self.phys_pipe_length / self.L) * self.N))
        self.ly = self.N
        self.nx, self.ny = self.lx + 1, self.ly + 1

    def _cylinder_grid_dims(self, mask_dtype):
        """Grid from pipe length and diameter in units of the radius; returns the F-ordered mask of the disc of N cells
        radius (opencl_dim.py:458-475, cython_dim.pyx:414-433)."""
        self.lx = int(np.ceil((self.phys_pipe_length / self.L) * self.N))
        self.ly = int(np.ceil((self.phys_diameter / self.L) * self.N))
        self.nx, self.ny = self.lx + 1, self.ly + 1
        mask = np.zeros((self.nx, self.ny), dtype=mask_dtype, order='F')
        xs, ys = disc_pixels(self.N * self.phys_cylinder_center[0] / self.L,
                             self.N * self.phys_cylinder_center[1] / self.L, self.N, (self.nx, self.ny))
        mask[xs, ys] = 1
        return mask

    def _density_ramp(self, order):
        """Sets and reports the boundary densities; returns (rho, zero): the linear ramp from inlet to outlet and the
        velocity of a fluid at rest, float32 (nx, ny) in the given memory order (opencl_dim.py:258-293)."""
        self.inlet_rho, self.outlet_rho = self._boundary_densities()
        self._say('inlet rho:', self.inlet_rho)
        self._say('outlet rho:', self.outlet_rho)
        i = np.arange(self.nx, dtype=np.float64)[:, None]
        ramp = self.inlet_rho - i * (self.inlet_rho - self.outlet_rho) / float(self.nx)
        rho = np.array(np.broadcast_to(ramp, (self.nx, self.ny)), dtype=np.float32, order=order)
        return rho, np.zeros((self.nx, self.ny), np.float32, order=order)
