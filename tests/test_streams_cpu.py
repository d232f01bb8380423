"""The child scripts of tests/test_gpu_streams.py without a GPU (tests/stream_scenarios.py): every child source compiles, defines the
scenarios the table lists for it and nothing else, and the table names every entry point whose stream order the GPU file is about."""
import ast

import pytest

import stream_scenarios as S


@pytest.mark.parametrize("child", sorted(S.CHILDREN))
def test_child_source_compiles_and_defines_its_scenarios(child):
    src = S.child_source(child)
    tree = ast.parse(src, filename="<%s>" % child)
    compile(src, "<%s>" % child, "exec")
    registered = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and
                  any(isinstance(d, ast.Name) and d.id == "scenario" for d in n.decorator_list)]
    listed = [name for name, (c, _) in S.SCENARIOS.items() if c == child]
    assert sorted(registered) == sorted(listed) and len(set(registered)) == len(registered), (registered, listed)
    assert 'CHILD = "%s"' % child in src
    # torch before the library: one HIP runtime in the process (tests/test_gpu_poisson.py, the device-source child)
    assert src.index("import torch") < src.index("from LB_D2Q9")
    assert "os.exec" not in src and "execv" not in src      # a process that has opened the GPU never replaces its program


def test_at_most_four_children():
    assert 1 <= len(S.CHILDREN) <= 4 and {c for c, _ in S.SCENARIOS.values()} == set(S.CHILDREN)


def test_the_table_names_every_entry_point():
    named = {e for _, entries in S.SCENARIOS.values() for e in entries}
    assert named == set(S.ENTRY_POINTS), (named ^ set(S.ENTRY_POINTS))
    # what the issue lists: the async halo copies, the graph capture, the forks to the edge / communication stream, the set calls
    # that join their members' streams, the timer and the tuner's events, lb_set_stream itself, and the device-pointer argument
    for e in ("lb_halo_export", "lb_halo_import", "ensure_graph", "vel_band_pass", "run_slab", "lb_run_batch", "lb_run_coupled",
              "lb_run_fluids", "lb_timer_start", "lb_timer_stop", "lb_autotune_quick", "lb_set_stream", "lb_set_force_field"):
        assert e in named, e


def _reachable_source(child, name):
    """The source of scenario `name` and of every function of its child (PRELUDE included) that it reaches by name, transitively."""
    src = S.PRELUDE + S.CHILDREN[child]
    funcs = {n.name: n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    seen, todo = set(), [name]
    while todo:
        f = todo.pop()
        if f in seen or f not in funcs:
            continue
        seen.add(f)
        todo += [n.id for n in ast.walk(funcs[f]) if isinstance(n, ast.Name)]
    return "\n".join(ast.get_source_segment(src, funcs[f]) for f in sorted(seen))


def test_every_scenario_uses_what_the_table_says():
    """The Python call behind each entry point occurs in the scenario the table lists it for: in its own body or in a function it
    reaches (not merely somewhere in the child)."""
    call = dict(lb_halo_export=("halo_export(", "DistributedSlab("), lb_halo_import=("halo_import(", "DistributedSlab("),
                ensure_graph=("V.K_STEP)",), vel_band_pass=("V.K_STEP3",), run_slab=("peer_connect(",), lb_run_batch=("lb_run_batch(",),
                lb_run_coupled=("lb_run_coupled(",), lb_run_fluids=("Shan_Chen_Fluids(",), lb_timer_start=("timer_start(",),
                lb_timer_stop=("timer_stop(",), lb_autotune_quick=("lb_autotune_quick(",), lb_set_stream=("use_stream(", "DistributedSlab("),
                lb_set_force_field=("lb_set_force_field(",))
    for name, (child, entries) in S.SCENARIOS.items():
        body = _reachable_source(child, name)
        assert "def %s()" % name in body, name
        for e in entries:
            assert any(c in body for c in call[e]), (name, e)
    # and the check can fail: a scenario that reaches no export does not pass for lb_halo_export
    assert "halo_export(" not in _reachable_source("SETS", "fluids_on_one_external_stream")
    assert "halo_export(" not in _reachable_source("FORKS", "timer_on_the_stream")


def test_use_stream_refuses_the_default_streams_handle():
    """Handle 0 is the legacy default stream, which lb_set_stream reads as `own stream`: refused before the library is asked."""
    from LB_D2Q9.simulation import Simulation
    sim = Simulation.__new__(Simulation)            # (no handle: the check comes first)
    sim._h = None
    with pytest.raises(ValueError):
        sim.use_stream(0)
