"""Noisy strains on a shared nutrient in numpy, pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/D2Q9_multifield_diffusion.cl computes per iteration of advecting_range_expansion/stochastic_nutrients.py's run loop,
written for whole arrays: NP strains and the nutrient behind them, NP + 1 scalar lattices (scalar_model.ScalarModel: streaming, the
'open' and 'periodic' families, the edge state, feq with the constant 3) in one box.
  update_hydro        rho_i = sum_k f_ik, left to right; rho_i < zero_cutoff or NaN -> 0
  collide_particles   c = the nutrient's rho; strain i: react_i = (G_i rho_i) c + sqrt((Dg_i rho_i) c) z_i + ((Dg_i c) / 4)(z_i z_i - 1),
                      f_ik = f_ik (1 - omega_i) + omega_i feq_ik + w_k react_i; the nutrient takes - sum_i react_i, accumulated in the
                      strains' order; a link becomes 0 where its member's rho < zero_cutoff, where the new value < 0 or where it is NaN
Every operation is one operation in `dtype` in the reference's order, but the Milstein term: the reference's `4.` and `1.` are double
literals, so it forms ((Dg c) / 4.)(z z - 1.) and the sum with the first term in double and rounds once -- the float32 model does
exactly that (milstein='double', the default) or keeps every operation in float32 as the engine does (milstein='single').
z_i of a collision: the strain's noise_field if one is set, else the stream (noise_model.normals64, rounded to float32) under the
strain's seed at its noise counter t; a strain with Dg == 0 draws nothing and its t does not move.

Arrays: f, feq (nx, ny, NP + 1, 9), rho (nx, ny, NP + 1), u, v (nx, ny).
"""
import numpy as np

from noise_model import normals64
from scalar_model import F, ScalarModel


class ExpansionModel(object):
    def __init__(self, nx, ny, omegas, omega_nutrient, Gs, Dgs=None, seeds=None, zero_cutoff=0.01, bc="open", dtype=F, milstein="double"):
        T = self.T = np.dtype(dtype).type
        self.nx, self.ny, self.np_, self.bc, self.milstein = int(nx), int(ny), len(omegas), bc, milstein
        self.members = [ScalarModel(nx, ny, om, 0., bc, dtype) for om in list(omegas) + [omega_nutrient]]
        self.G = [T(F(g)) for g in Gs]
        self.Dg = [T(F(d)) for d in (Dgs if Dgs is not None else [0.] * self.np_)]
        self.seeds = [int(s) for s in (seeds if seeds is not None else range(self.np_))]
        self.t = [0] * self.np_
        self.noise_fields = [None] * self.np_
        self.cut = T(F(zero_cutoff))
        self.w = self.members[0].w

    # -- state ---------------------------------------------------------------------------------------------------------------
    def set_f(self, f):
        for i, m in enumerate(self.members):
            m.set_f(np.asarray(f)[:, :, i, :])

    def set_fields(self, rho, u, v):
        for i, m in enumerate(self.members):
            m.set_fields(np.asarray(rho)[:, :, i], u, v)

    def set_edge_state(self, e):
        for m, row in zip(self.members, e):
            m.set_edge_state(row)

    def zero_edge_state(self):
        for m in self.members:
            m.frozen[...] = 0

    def get_fields(self):
        st = lambda k: np.stack([getattr(m, k) for m in self.members], axis=2)
        return dict(f=st("f"), feq=st("feq"), rho=st("rho"), u=self.members[0].u, v=self.members[0].v)

    # -- the phases -----------------------------------------------------------------------------------------------------------
    def move(self):
        for m in self.members:
            m.move()

    def update_hydro(self):
        for m in self.members:
            m.update_hydro()
            with np.errstate(invalid="ignore"):
                m.rho = np.where((m.rho < self.cut) | np.isnan(m.rho), self.T(0.), m.rho)

    def update_feq(self):
        for m in self.members:
            m.update_feq()

    def _react(self, i, rho, c):
        T = self.T
        growth = self.G[i] * rho * c
        if self.Dg[i] == 0:
            return growth
        z = self.noise_fields[i] if self.noise_fields[i] is not None else normals64(self.nx, self.ny, self.seeds[i], self.t[i]).astype(F)
        z = np.asarray(z, T)
        self.t[i] += 1
        with np.errstate(invalid="ignore"):
            kick = np.sqrt(self.Dg[i] * rho * c) * z
            if T == F and self.milstein == "double":
                D = np.float64
                mil = ((self.Dg[i] * c).astype(D) / D(4.)) * ((z * z).astype(D) - D(1.))
                fluct = (kick.astype(D) + mil).astype(F)
            else:
                mil = (self.Dg[i] * c * T(0.25)) * (z * z - T(1.))
                fluct = kick + mil
            return growth + fluct

    def collide_particles(self):
        """Returns the links set to 0, (nx, ny, NP + 1, 9) bool."""
        T = self.T
        c = self.members[-1].rho
        eaten = np.zeros((self.nx, self.ny), T)
        zeroed = np.zeros((self.nx, self.ny, self.np_ + 1, 9), bool)
        for i, m in enumerate(self.members):
            if i < self.np_:
                react = self._react(i, m.rho, c)
                eaten = eaten - react
            else:
                react = eaten
            keep = T(1.) - m.omega
            with np.errstate(invalid="ignore"):
                for k in range(9):
                    new = m.f[:, :, k] * keep + m.omega * m.feq[:, :, k]
                    new = new + self.w[k] * react
                    zero = (m.rho < self.cut) | (new < 0) | np.isnan(new)
                    zeroed[:, :, i, k] = zero
                    m.f[:, :, k] = np.where(zero, T(0.), new)
        return zeroed

    def step(self):
        self.move()
        self.update_hydro()
        self.update_feq()
        return self.collide_particles()

    def run(self, n):
        for _ in range(int(n)):
            self.step()


def from_fixture(d, dtype=F, milstein="double", stored_normals=False):
    """The model at a run fixture's start (tools/make_golden_expansion.py); stored_normals: step t draws d['z'][t]."""
    m = ExpansionModel(int(d["nx"]), int(d["ny"]), d["omega"], float(d["omega_nutrient"]), d["G"], d["Dg"], [int(s) for s in d["seeds"]],
                       float(d["zero_cutoff"]), str(d["bc"]), dtype, milstein)
    m.set_f(d["f0"])
    if int(d["edge_zero"]):
        m.zero_edge_state()
    nf = len(m.members)
    m.set_fields(np.zeros((m.nx, m.ny, nf), np.float32), d["u"], d["v"])
    return m
