"""The public surface of the Python package is fixed: tools/dump_python_api.py on the working tree gives what it gave on the commit
before the wrappers were folded onto ``_handle.Handle`` (tests/golden/python_api.json: names, signatures, methods and properties of
classes with inherited ones, values of constants, and the private names tests reach into).  Needs neither a GPU nor the built library."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dumps():
    spec = importlib.util.spec_from_file_location("dump_python_api", os.path.join(ROOT, "tools", "dump_python_api.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "python_api.json")) as f:
        return json.load(f), json.loads(json.dumps(tool.dump(), sort_keys=True))


def test_public_surface_is_the_fixture(dumps):
    want, got = dumps
    # a module the fixture does not know may only be a private one (``_handle``): it adds no public name
    added = set(got["modules"]) - set(want["modules"])
    assert all(name.rpartition(".")[2].startswith("_") for name in added), sorted(added)
    for module, names in want["modules"].items():
        assert module in got["modules"], f"module {module} is gone"
        have = got["modules"][module]
        assert sorted(have) == sorted(names), (module, sorted(set(names) ^ set(have)))
        for name, described in names.items():
            assert have[name] == described, (module, name, described, have[name])


def test_documented_methods_stay_documented(dumps):
    want, got = dumps
    assert len(want["documented"]) == 15
    for cls, names in want["documented"].items():
        missing = sorted(set(names) - set(got["documented"].get(cls, ())))
        assert not missing, f"{cls}: no docstring any more on {missing}"
