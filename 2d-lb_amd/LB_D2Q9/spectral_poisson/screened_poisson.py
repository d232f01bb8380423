"""The screened Poisson equation ``(1 - lam^2 laplace) phi = charge`` in a periodic box, solved spectrally: the surface of the
reference's ``LB_D2Q9.spectral_poisson.screened_poisson.Screened_Poisson`` on an ``lb_spectral`` of liblbhip (include/lb_hip.h).

The reference drives three gpyfft plans and multiplies whole arrays between them, waiting after each; here every method is one to
three HIP launches of the library's own transform (axis lengths ``2^a 3^b 5^c <= 4096``; anything else raises ``LbError`` with the
rule).  Conventions are the reference's: ``freq_X, freq_Y`` are the integer wave indices ``L * fftfreq(n, d=dx)`` (the Nyquist index
of an even axis is ``-n/2``), ``rescaling = 1 / (lam^2 (freq_X^2 + freq_Y^2) + 1)``, the gradient multipliers are ``2 pi i freq``,
and the inverse transform carries ``1 / (nx ny)``.  ``charge``, ``xgrad``, ``ygrad`` are live views of the device arrays:
``.get()`` / ``np.asarray`` give complex64 ``(nx, ny)`` Fortran-ordered host copies, ``.set(a)`` uploads one.

Repairs: ``cl_context`` / ``cl_queue`` are gone (``device`` selects the GPU); ``solve_and_update_grad_fields`` is
the fused three-launch solve, bitwise what ``fft_and_screen(); update_grad_fields()`` leaves.
"""
import ctypes as ct

import numpy as np

from .. import _native
from .._native import check

CHARGE, XGRAD, YGRAD = 0, 1, 2


class SpectralField(object):
    """A named view of one of the solver's device arrays."""

    def __init__(self, owner, which):
        self._owner, self._which = owner, which

    def get(self):
        return self._owner._read(self._which)

    def set(self, a):
        self._owner._write(self._which, a)

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a if dtype is None else a.astype(dtype)

    @property
    def real(self):
        return self.get().real

    @property
    def imag(self):
        return self.get().imag


class Screened_Poisson(object):
    def __init__(self, charge_cpu, lam=1., dx=1., device=0):
        charge_cpu = np.asarray(charge_cpu).astype(np.complex64, order='F')
        if charge_cpu.ndim != 2:
            raise ValueError("the charge is a two-dimensional (nx, ny) array")
        self.nx, self.ny = charge_cpu.shape
        self.lam, self.dx, self.device = lam, dx, int(device)
        self._lib = _native.lib()
        self._h = ct.c_void_p()
        check(self._lib.lb_spectral_create(self.nx, self.ny, self.device, float(lam), ct.byref(self._h)))

        Lx, Ly = self.dx * self.nx, self.dx * self.ny
        freq_x = Lx * np.fft.fftfreq(self.nx, d=dx)
        freq_y = Ly * np.fft.fftfreq(self.ny, d=dx)
        freq_Y, freq_X = np.meshgrid(freq_y, freq_x)
        self.freq_X, self.freq_Y = np.asfortranarray(freq_X), np.asfortranarray(freq_Y)
        self.rescaling = 1. / (self.lam ** 2 * (self.freq_X ** 2 + self.freq_Y ** 2) + 1.)

        self.charge = SpectralField(self, CHARGE)
        self.charge.set(charge_cpu)
        self.xgrad = self.ygrad = None
        self.xgrad_rescale = self.ygrad_rescale = None

    # -- lifetime ------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lb_spectral_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host <-> device: (nx, ny) Fortran order is the device's [ny][nx] ---------------------------------------------------------
    def _read(self, which):
        out = np.zeros((self.nx, self.ny), np.complex64, order='F')
        check(self._lib.lb_spectral_get(self._h, which, out.ctypes.data))
        return out

    def _write(self, which, a):
        a = np.asarray(a)
        if a.shape != (self.nx, self.ny):
            raise ValueError("expected shape %s, got %s" % ((self.nx, self.ny), a.shape))
        a = np.asfortranarray(a.astype(np.complex64))
        check(self._lib.lb_spectral_set(self._h, which, a.ctypes.data, 0))

    def set_lambda(self, lam):
        check(self._lib.lb_spectral_set_lambda(self._h, float(lam)))
        self.lam = lam
        self.rescaling = 1. / (self.lam ** 2 * (self.freq_X ** 2 + self.freq_Y ** 2) + 1.)

    # -- the reference's methods ---------------------------------------------------------------------------------------------
    def fft_and_screen(self):
        check(self._lib.lb_spectral_transform(self._h, CHARGE, 1))
        check(self._lib.lb_spectral_screen(self._h))

    def inverse_fft(self):
        check(self._lib.lb_spectral_transform(self._h, CHARGE, 0))

    def create_grad_fields(self):
        self.xgrad, self.ygrad = SpectralField(self, XGRAD), SpectralField(self, YGRAD)
        self.xgrad_rescale = 2 * np.pi * 1.0j * self.freq_X
        self.ygrad_rescale = 2 * np.pi * 1.0j * self.freq_Y

    def update_grad_fields(self):
        """Requires fft_and_screen to have been run first."""
        if self.xgrad is None:
            raise RuntimeError("create_grad_fields() first")
        check(self._lib.lb_spectral_grad_multiply(self._h))
        check(self._lib.lb_spectral_transform(self._h, XGRAD, 0))
        check(self._lib.lb_spectral_transform(self._h, YGRAD, 0))

    def solve_and_update_grad_fields(self):
        """Solve the screened Poisson equation and leave the gradient fields: three fused launches."""
        if self.xgrad is None:
            raise RuntimeError("create_grad_fields() first")
        check(self._lib.lb_spectral_solve(self._h))
