"""The child script of tests/test_gpu_nutrient.py's stream test (test infrastructure; not a test module): tests/stream_scenarios.py's
method -- PRELUDE, the scenarios, EPILOGUE, run by a fresh `python`; a bounded delay on a torch side stream S, the chain under test
behind it without a host wait, one synchronisation, a bitwise comparison with a twin that waits after every call -- for
lb_run_nutrient.

The chain: the population's handle on S, the nutrient's on its own stream, the solver on its own.  Behind the delay on S: run(3); an
lb_spectral_solve on the SOLVER's stream, which must wait for the run that borrowed its arrays (sp_return); run(4), which must wait
for that solve (sp_borrow).  (psi and F are made before the delay starts, by an lb_update_forces_nutrient: an allocation is no
enqueue-only call.)  (No control of its own, as for the coupled set: these handles take no device buffer a torch
op could poison -- a scalar lattice has no device-pointer setter for rho; the device pointer in this chain is the solver's charge,
set with on_device = 1 before the delay starts.)
"""
from stream_scenarios import EPILOGUE, PRELUDE  # noqa: F401

NUTRIENT = r'''
CHILD = "NUTRIENT"


@scenario
def nutrient_set_on_an_external_stream():
    from LB_D2Q9.nutrient_set import Nutrient_Set
    nx, ny = 30, 18
    rng = np.random.default_rng(90)
    rho = np.stack([0.7 + 0.3 * rng.random((nx, ny)), 0.6 + 0.3 * rng.random((nx, ny))], axis=2)
    f0 = (W[None, None, None, :] * rho[:, :, :, None] * (1 + 0.02 * rng.standard_normal((nx, ny, 2, 9)))).astype(np.float32)
    charge = torch.tensor(rng.standard_normal((ny, nx, 2)).astype(np.float32), device=DEV)
    KEYS = ("f", "rho", "u", "v", "psi", "pseudo_force_x", "pseudo_force_y")

    def make():
        s = Nutrient_Set(nx, ny, 0.8, 1.25, lam=1., dx=0.1)
        s.set_params(G=0.01, scale=-0.05, clumpy=True, rho_o=1., G_chen=-1.)
        s.set_f(f0)
        s.update_hydro()
        s.update_forces()
        torch.cuda.synchronize()
        _native.check(L.lb_spectral_set(s.solver._h, 0, charge.data_ptr(), 1))
        return s

    tw = make()
    tw.run(3)
    _native.check(L.lb_spectral_solve(tw.solver._h))
    torch.cuda.synchronize()
    tw.run(4)
    want = tw.get_fields(KEYS)
    tw.close()

    S = SIDE[0]
    s = make()
    s.members[0].use_stream(S.cuda_stream)
    torch.cuda.synchronize()
    d = Delay(S)
    s.run(3, wait=False)
    _native.check(L.lb_spectral_solve(s.solver._h))
    s.run(4, wait=False)
    d.done()
    torch.cuda.synchronize()
    d.check("lb_run_nutrient")
    got = s.get_fields(KEYS)
    s.members[0].use_stream(None)
    s.close()
    assert_same(got, want, "lb_run_nutrient, the population on S")
'''
