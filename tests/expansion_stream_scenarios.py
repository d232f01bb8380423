"""The child script of tests/test_gpu_expansion.py's stream test (test infrastructure; not a test module): tests/stream_scenarios.py's
method -- PRELUDE, the scenario, EPILOGUE, run by a fresh `python`; a bounded delay on a torch side stream S, the chain under test
behind it without a host wait, one synchronisation, a bitwise comparison with a twin that waits after every call -- for
lb_run_expansion.

The chain: two noisy strains and the nutrient; the NUTRIENT's handle on S, the strains on their own streams.  Behind the delay on S: a
plain run(3) of the nutrient alone on S; lb_run_expansion(4) on the first strain's stream, which must wait for it (SetScope::join); a run(2)
of the nutrient alone on S again, which must wait for the set's launches (SetScope::release).  (No control of its own, as for the coupled
set: these handles take no device buffer a torch op could poison.)
"""
from stream_scenarios import EPILOGUE, PRELUDE  # noqa: F401

EXPANSION = r'''
CHILD = "EXPANSION"


@scenario
def expansion_set_with_the_nutrient_on_an_external_stream():
    from LB_D2Q9.expansion_set import Expansion_Set
    nx, ny = 37, 23
    rng = np.random.default_rng(91)
    rho = np.stack([0.3 + 0.2 * rng.random((nx, ny)), 0.2 + 0.2 * rng.random((nx, ny)), 0.7 + 0.3 * rng.random((nx, ny))], axis=2)
    f0 = (W[None, None, None, :] * rho[:, :, :, None] * (1 + 0.02 * rng.standard_normal((nx, ny, 3, 9)))).astype(np.float32)
    u, v = (0.03 * rng.standard_normal((2, nx, ny))).astype(np.float32)

    def make():
        s = Expansion_Set(nx, ny, (1.1, 0.9), 1.3, (0.01, 0.014), bc="open", zero_cutoff=0.01)
        s.set_noise((2.0e-3, 1.0e-3), seed=5)
        s.set_fields(np.ones((nx, ny, 3), np.float32), u, v)
        s.set_f(f0)
        return s

    def fields(s):
        out = s.get_fields(("f", "rho"))
        out["t"] = np.array([n[2] for n in s.noise()])
        return out

    tw = make()
    tw.nutrient.run(3)
    tw.run(4)
    tw.nutrient.run(2)
    want = fields(tw)
    tw.close()

    S = SIDE[0]
    s = make()
    s.nutrient.use_stream(S.cuda_stream)
    torch.cuda.synchronize()
    d = Delay(S)
    s.nutrient.run(3, wait=False)
    s.run(4, wait=False)
    s.nutrient.run(2, wait=False)
    d.done()
    torch.cuda.synchronize()
    d.check("lb_run_expansion")
    got = fields(s)
    s.nutrient.use_stream(None)
    s.close()
    assert_same(got, want, "lb_run_expansion, the nutrient on S")
'''
