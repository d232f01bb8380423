"""The noisy collision of a scalar lattice in numpy (test infrastructure; not a test module).

Two things:
  * Philox4x32-10 and the stream csrc/philox.h defines -- integers as uint64 arithmetic masked to 32 bits, the transcendental part
    (ln, sqrt, cos, sin) in float64: the yardstick the device's float32 normals are held to;
  * the reference's collide_particles_noisy_fisher (D2Q9_diffusion.cl:127-167) on top of the pull-form model of scalar_model.py:
        react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z;   f_k = f_k (1 - omega) + omega feq_k + w_k react;   f_k < 0 -> 0
    (a compare: NaN stays), every operation one float32 operation in the reference's order.

The stream: the four cells x = 4j .. 4j+3 of row y take the words r0 .. r3 of counter (j, y, t_lo, t_hi) under key (seed_lo, seed_hi);
u(r) = float(r >> 9) 2^-23 + 2^-24; cells 0, 1 get R cos(theta), R sin(theta) with R = sqrt(-2 ln u(r0)), theta = 2 pi u(r1); cells 2, 3
the same from r2, r3.
"""
import numpy as np

from scalar_model import F, ScalarModel

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two; returns the four output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & M32 for c in counter])
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2             # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform(r):
    """float(r >> 9) 2^-23 + 2^-24: exact in float32 (and so in float64)"""
    return (np.asarray(r, np.uint64) >> np.uint64(9)).astype(np.float64) * 2. ** -23 + 2. ** -24


def normals64(nx, ny, seed, t):
    """The (nx, ny) float64 normals of noise counter t under `seed`."""
    seed, t = int(seed), int(t)
    lanes = (nx + 3) // 4
    j, y = np.meshgrid(np.arange(lanes, dtype=np.uint64), np.arange(ny, dtype=np.uint64), indexing="ij")
    r = philox4x32_10((j, y, t & 0xFFFFFFFF, t >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((4 * lanes, ny), np.float64)
    for h in range(2):
        radius = np.sqrt(-2. * np.log(uniform(r[2 * h])))
        theta = 2. * np.pi * uniform(r[2 * h + 1])
        z[2 * h::4] = radius * np.cos(theta)
        z[2 * h + 1::4] = radius * np.sin(theta)
    return z[:nx]


def normals32(nx, ny, seed, t):
    return normals64(nx, ny, seed, t).astype(F)


class NoisyScalarModel(ScalarModel):
    """ScalarModel with the noisy collision.  z of each collision: noise_field if one is set (used once per collision, as the un-fused
    API does), else the stream at the model's counter t, rounded to float32; t counts the collisions."""

    def __init__(self, nx, ny, omega, G=0., Dg=0., seed=0, bc="open", dtype=F):
        super(NoisyScalarModel, self).__init__(nx, ny, omega, G, bc, dtype)
        self.Dg, self.seed, self.t = self.T(F(Dg)), int(seed), 0
        self.noise_field = None

    def collide_particles(self):
        if self.Dg == 0:
            return super(NoisyScalarModel, self).collide_particles()
        T = self.T
        z = self.noise_field if self.noise_field is not None else normals64(self.nx, self.ny, self.seed, self.t).astype(F)
        z = np.asarray(z, T)
        self.t += 1
        keep, rho = T(1.) - self.omega, self.rho
        with np.errstate(invalid="ignore"):
            grow = self.G * rho * (T(1.) - rho)
            kick = np.sqrt(self.Dg * rho * (T(1.) - rho)) * z
            react = grow + kick
            for k in range(9):
                new = self.f[:, :, k] * keep + self.omega * self.feq[:, :, k]
                new = new + self.w[k] * react
                self.f[:, :, k] = np.where(new < 0, T(0.), new)
