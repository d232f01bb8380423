"""The package keeps the surface it had one commit earlier: every class's public names and every public callable's signature.

When the Python package was folded -- one row per handle kind, one signature table for the binding, one base class for the lattice
sets, one for the forced-fluid drop-ins -- no class was to gain or lose a public name and no signature was to change.
package_surface.json holds what the commit before that fold showed:

  for every class defined in a module of LB_D2Q9: the public names dir() lists (inherited ones included, so a method that moved into
  a base class still counts for every subclass), str(inspect.signature(...)) of each one that is callable, and that of __init__;
  for every module: its public functions and their signatures.

Importing the modules needs neither a GPU nor the library.  record() wrote the table; the tests compare class by class and module by
module and name what differs.  Classes and modules the table does not hold are the fold's own (the shared bases, the kind table): the
tests do not look at them, but what a class of the table inherits from them they do see.
"""
import importlib
import inspect
import json
import os

import pytest

from conftest import ROOT

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "package_surface.json")
PACKAGE = os.path.join(ROOT, "2d-lb_amd", "LB_D2Q9")


def module_names():
    names = []
    for base, dirs, files in os.walk(PACKAGE):
        dirs[:] = sorted(d for d in dirs if d != "__pycache__")
        for f in sorted(files):
            if f.endswith(".py"):
                parts = os.path.relpath(os.path.join(base, f), os.path.dirname(PACKAGE))[:-3].split(os.sep)
                names.append(".".join(parts[:-1] if parts[-1] == "__init__" else parts))
    return sorted(names)


def signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):             # (a builtin without a text signature)
        return "?"


def class_surface(cls):
    """{public name: its signature, or None where it is not callable}, and the constructor's under '__init__'."""
    out = {"__init__": signature(cls.__init__)}
    for name in dir(cls):
        if not name.startswith("_"):
            attr = getattr(cls, name)
            out[name] = signature(attr) if callable(attr) else None
    return out


def surface():
    classes, functions = {}, {}
    for mod_name in module_names():
        mod = importlib.import_module(mod_name)
        functions[mod_name] = {}
        for name, obj in sorted(vars(mod).items()):
            if getattr(obj, "__module__", None) != mod_name or name.startswith("_"):
                continue
            if inspect.isclass(obj):
                classes["%s.%s" % (mod_name, name)] = class_surface(obj)
            elif inspect.isfunction(obj):
                functions[mod_name][name] = signature(obj)
    return {"classes": classes, "functions": functions}


def table():
    if not os.path.exists(TABLE):               # (only before record() has run: the test of the table's size fails then)
        return {"classes": {}, "functions": {}}
    with open(TABLE) as fh:
        return json.load(fh)


def differences(got, want):
    """What differs between two {name: signature} dicts, in words."""
    out = ["lost %s" % k for k in sorted(set(want) - set(got))] + ["gained %s" % k for k in sorted(set(got) - set(want))]
    return out + ["%s%s was %s%s" % (k, got[k], k, want[k]) for k in sorted(set(got) & set(want)) if got[k] != want[k]]


@pytest.fixture(scope="module")
def now():
    return surface()


def test_the_table_is_the_size_it_was_recorded_at():
    """36 classes with 553 public names among them, inherited ones counted in every subclass."""
    classes = table()["classes"]
    assert len(classes) == 36
    assert sum(len(c) - 1 for c in classes.values()) == 553          # (- 1: '__init__' is no public name)


def test_no_class_or_module_went(now):
    want = table()
    assert sorted(set(want["classes"]) - set(now["classes"])) == []
    assert sorted(set(want["functions"]) - set(now["functions"])) == []


@pytest.mark.parametrize("name", sorted(table()["classes"]))
def test_class_keeps_its_public_names_and_signatures(now, name):
    assert name in now["classes"], "%s is gone" % name
    assert differences(now["classes"][name], table()["classes"][name]) == [], name


@pytest.mark.parametrize("name", sorted(table()["functions"]))
def test_module_keeps_its_public_functions(now, name):
    assert name in now["functions"], "%s is gone" % name
    assert differences(now["functions"][name], table()["functions"][name]) == [], name


def record():
    """Writes package_surface.json.  Run by hand from a checkout of the parent commit with this file copied into tests/:
        python tests/test_package_surface_cpu.py
    The committed table was recorded at 39558e5 ("One row per handle kind: fold each physics' host code into its unit"), the commit
    before the package was folded."""
    out = surface()
    with open(TABLE, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import conftest  # noqa: F401  (puts the package on the path)
    out = record()
    print("%d classes, %d public names, %d modules recorded"
          % (len(out["classes"]), sum(len(c) - 1 for c in out["classes"].values()), len(out["functions"])))
