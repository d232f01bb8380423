"""A scalar lattice with the noisy collision: ``NoisySimulation`` is ``Simulation(..., semantics='diffusion')`` plus the four calls
of the library's noise entry points (``lb_set_noise`` ...: include/lb_hip.h, csrc/philox.h).  ``Simulation`` keeps the public surface
it has; a checkpoint written by either class carries the noise (``noise = [Dg bits, seed, t]``, when Dg != 0) and either class
restores it: ``NoisySimulation.from_checkpoint(path)`` gives the calls below on the restored handle."""
import numpy as np

from .simulation import Simulation


class NoisySimulation(Simulation):
    def __init__(self, nx, ny, omega, bc="open", semantics="diffusion", **kwargs):
        if semantics != "diffusion":
            raise ValueError("the noisy collision is for scalar lattices on their own: semantics='diffusion'")
        super(NoisySimulation, self).__init__(nx, ny, omega, bc=bc, semantics=semantics, **kwargs)

    def set_noise(self, Dg, seed=0):
        """The noisy collision (D2Q9_diffusion.cl:127-167): react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z, f_k < 0 -> 0, with z a
        standard normal per cell and collision drawn inside the kernels from a counter-based stream (Philox4x32-10 under the 64-bit
        `seed`).  Dg > 0 switches it on and resets the noise counter; 0 switches back to the plain cell.  run(), the screened wave's
        run and collide_particles() honour it.  rho outside [0, 1] gives NaN, as in the reference: check() counts such cells."""
        self._set_noise(Dg, seed)

    def noise(self):
        """(Dg, seed, t): t = the noise counter, the number of noisy collisions since set_noise."""
        return self._noise()

    def noise_fill(self, t):
        """The (nx, ny) float32 normals the kernels draw at noise counter t under the handle's seed (lb_noise_fill)."""
        return self._noise_fill(t)

    def set_noise_field(self, z):
        """A supplied (nx, ny) field of normals that collide_particles() uses in place of the stream (the reference's random_normal
        buffer); None drops it.  While one is set run() refuses: a field is never used twice.  Not part of a checkpoint."""
        self._set_noise_field(None if z is None else np.asarray(z))
