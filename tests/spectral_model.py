"""A numpy model of the spectral screened-Poisson solve and of the scalar Fisher lattice coupled to it (test infrastructure; not a test
module).

What the reference's spectral_poisson/screened_poisson.py computes, for whole arrays: with the integer wave indices kx, ky of
numpy's fftfreq (the Nyquist index of an even axis is -n/2),

    C = fft2(charge) / (lam^2 (kx^2 + ky^2) + 1)          fft_and_screen
    xgrad = ifft2(2 pi i kx C), ygrad = ifft2(2 pi i ky C)   update_grad_fields (the inverse carries 1 / (nx ny))

in complex128 or complex64 (numpy >= 2 transforms single precision in single precision), and reaction_diffusion/
screened_poisson_waves.py's step on top of ScalarModel: move, update_hydro, u = scale Re xgrad and v = scale Re ygrad
(scale = -vc delta_t / delta_x), update_feq, collide_particles_fisher.

stockham(): the device's transform restated -- the same passes over the same indices (csrc/kernels_spectral.h: sp_pass) with numpy's
arithmetic --, so that the index scheme is checked on a host against numpy's fft for every radix mix.

Arrays are (nx, ny), x first, as everywhere in the package.
"""
import numpy as np

from scalar_model import ScalarModel

F = np.float32


def wave_index(n):
    """The integers n * fftfreq(n): 0 ... ceil(n/2) - 1, -floor(n/2) ... -1."""
    return np.rint(np.fft.fftfreq(n, d=1. / n)).astype(np.int64)


def wave_grids(nx, ny):
    return np.meshgrid(wave_index(nx), wave_index(ny), indexing='ij')


def rescaling(nx, ny, lam):
    kx, ky = wave_grids(nx, ny)
    return 1. / (float(lam) ** 2 * (kx ** 2 + ky ** 2) + 1.)


def solve(charge, lam, dtype=np.complex128):
    """(screened spectrum, xgrad, ygrad), each (nx, ny) of `dtype`."""
    ctype = np.dtype(dtype)
    rtype = np.float32 if ctype == np.complex64 else np.float64
    charge = np.asarray(charge).astype(ctype)
    nx, ny = charge.shape
    kx, ky = wave_grids(nx, ny)
    spec = (np.fft.fft2(charge) * rescaling(nx, ny, lam).astype(rtype)).astype(ctype)
    mx = (2 * np.pi * 1.0j * kx).astype(ctype)
    my = (2 * np.pi * 1.0j * ky).astype(ctype)
    xg = np.fft.ifft2((spec * mx).astype(ctype)).astype(ctype)
    yg = np.fft.ifft2((spec * my).astype(ctype)).astype(ctype)
    assert spec.dtype == ctype and xg.dtype == ctype
    return spec, xg, yg


def round_trip(charge, dtype=np.complex128):
    ctype = np.dtype(dtype)
    return np.fft.ifft2(np.fft.fft2(np.asarray(charge).astype(ctype))).astype(ctype)


def radix_passes(n):
    """The passes csrc/spectral_plan.cpp gives an axis: 5s, 3s, 4s, a 2."""
    out = []
    for r in (5, 3, 4, 2):
        while n % r == 0:
            out.append(r)
            n //= r
    assert n == 1
    return out


def stockham(x, radices=None):
    """The forward transform of a 1-D complex128 array by the device's passes: butterfly t = p s + q reads src[q + s p + k m],
    k < r, m = n / r, and writes dst[q + s (r p + j)] = (DFT_r a)_j exp(-2 pi i p s j / n)."""
    x = np.asarray(x, np.complex128)
    n = len(x)
    radices = radix_passes(n) if radices is None else radices
    tw = np.exp(-2j * np.pi * np.arange(n) / n)
    s = 1
    for r in radices:
        m = n // r
        y = np.empty_like(x)
        dft = np.exp(-2j * np.pi * np.outer(np.arange(r), np.arange(r)) / r)
        for t in range(m):
            p, q = divmod(t, s)
            a = np.array([x[q + s * p + k * m] for k in range(r)])
            b = dft @ a
            for j in range(r):
                y[q + s * (r * p + j)] = b[j] * tw[p * s * j]
        x, s = y, s * r
    return x


class ScreenedFisherModel(ScalarModel):
    """Screened_Fisher_Wave's step; `scale` = -vc delta_t / delta_x, a float32 like the entry points' argument."""

    def __init__(self, nx, ny, omega, G, lam, scale, bc="open", dtype=F):
        super(ScreenedFisherModel, self).__init__(nx, ny, omega, G=G, bc=bc, dtype=dtype)
        self.lam = float(lam)
        self.scale = self.T(F(scale))
        self.ctype = np.complex64 if self.T == F else np.complex128

    def update_u_and_v(self):
        _, xg, yg = solve(self.rho, self.lam, self.ctype)
        self.u = (self.scale * xg.real).astype(self.T)
        self.v = (self.scale * yg.real).astype(self.T)

    def redo_initial_condition(self, rho):
        self.rho = np.array(rho, dtype=self.T)
        self.update_u_and_v()
        self.update_feq()
        self.set_f(self.feq.copy())

    def step(self):
        self.move()
        self.update_hydro()
        self.update_u_and_v()
        self.update_feq()
        self.collide_particles()


def fisher_lattice_parameters(Lx, Ly, vc, time_prefactor, N):
    """What the fixtures' header records: the arithmetic of screened_fisher_parameters, restated (the package's is tested against
    hand values and against this)."""
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    cs = F(1. / np.sqrt(3))
    lb_D = F(.25 * (delta_t / delta_x ** 2))
    omega = F((.5 + lb_D / cs ** 2) ** -1.)
    return dict(nx=int(np.round(N * Lx)), ny=int(np.round(N * Ly)), omega=omega, lb_G=F(1. * delta_t),
                scale=F(-vc * (delta_t / delta_x)), delta_x=delta_x, delta_t=delta_t)


def noisy_droplet(nx, ny, N, R0, seed, amplitude=0.05):
    """exp(-(X^2 + Y^2) / R0^2) around (nx // 2, ny // 2), X, Y in units of N cells, times 1 + amplitude x a seeded normal draw."""
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    Xd, Yd = (X - nx // 2) / float(N), (Y - ny // 2) / float(N)
    rho = np.exp(-(Xd ** 2 + Yd ** 2) / R0 ** 2)
    rng = np.random.RandomState(seed)
    return (rho * (1. + amplitude * rng.standard_normal((nx, ny)))).astype(F)
