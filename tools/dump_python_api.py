#!/usr/bin/env python3
"""The public surface of the Python package as sorted JSON: for every module of ``gpusorting_amd`` its public names; for functions
their signature; for classes their public methods and properties (inherited ones included) with signatures; for ints, strings, tuples
and dicts of those, the value; and the three privately named things the tests reach into.  Under ``"documented"`` it lists, for the
handle classes, the public methods and properties that carry a docstring (names only: no docstring text is written).

    python tools/dump_python_api.py [OUT.json]        # stdout without an argument

Needs neither a GPU nor the built library; nothing in the dump depends on either or on the torch version.
tests/golden/python_api.json is this dump of the commit before the wrappers were folded onto ``_handle.Handle``;
tests/test_python_api_cpu.py compares the working tree against it.
"""
from __future__ import annotations

import importlib
import inspect
import json
import pkgutil
import sys
import types
from pathlib import Path

ROOT = str(Path(__file__).resolve().parent.parent)
sys.path.insert(0, ROOT)

PACKAGE = "gpusorting_amd"
HANDLE_CLASSES = {"segsort": "SegmentedSort", "segsort16": "SegmentedSort16", "rowsort": "RowSort", "rowsort16": "RowSort16",
                  "sort16": "Sort16", "topk": "TopK", "topk16": "TopK16", "segtopk": "SegmentedTopK", "segtopk16": "SegmentedTopK16",
                  "unique": "Unique", "unique16": "Unique16", "unique64": "Unique64", "reduce": "ReduceByKey", "reduce64": "ReduceByKey64",
                  "search": "SortedSearch"}
PRIVATE_USED_BY_TESTS = {"functional": ("_segtopk_cache", "_search_cache", "_seg_sorter")}


def _signature(obj) -> str:
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return "<no signature>"


def _plain(v):
    """``v`` as JSON if it is an int, a string, or a tuple or dict of those; ValueError otherwise."""
    if isinstance(v, str):
        return v.replace(ROOT, "<root>")  # a path inside the checkout: the same dump wherever the checkout lies
    if isinstance(v, (bool, int)):
        return v
    if isinstance(v, tuple):
        return {"tuple": [_plain(x) for x in v]}
    if isinstance(v, dict):
        return {"dict": {json.dumps(_plain(k)): _plain(x) for k, x in v.items()}}
    raise ValueError(type(v).__name__)


def _members(cls) -> dict:
    out = {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, property):
            out[name] = "property"
        elif isinstance(raw, (staticmethod, classmethod)):
            out[name] = type(raw).__name__ + _signature(raw.__func__)
        elif inspect.isfunction(raw):
            out[name] = _signature(raw)
        else:
            try:
                out[name] = {"value": _plain(raw)}
            except ValueError:
                out[name] = type(raw).__name__
    return out


def _describe(obj):
    if inspect.isclass(obj):
        return {"class": _members(obj)}
    if inspect.isfunction(obj):
        return {"function": _signature(obj)}
    try:
        return {"value": _plain(obj)}
    except ValueError:
        return {"other": type(obj).__name__}


def _documented(cls) -> list:
    names = []
    for name in dir(cls):
        raw = inspect.getattr_static(cls, name)
        if not name.startswith("_") and (isinstance(raw, property) or inspect.isfunction(raw)) and getattr(raw, "__doc__", None):
            names.append(name)
    return names


def dump() -> dict:
    pkg = importlib.import_module(PACKAGE)
    names = [PACKAGE] + sorted(f"{PACKAGE}.{m.name}" for m in pkgutil.iter_modules(pkg.__path__))
    modules, documented = {}, {}
    for full in names:
        mod = importlib.import_module(full)
        short = full.partition(".")[2]
        entry = {}
        for name, obj in vars(mod).items():
            if name.startswith("_") or isinstance(obj, types.ModuleType) or name == "annotations":
                continue
            entry[name] = _describe(obj)
        for name in PRIVATE_USED_BY_TESTS.get(short, ()):
            obj = getattr(mod, name, None)
            entry[name] = {"function": _signature(obj)} if inspect.isfunction(obj) else {"other": type(obj).__name__}
        modules[full] = entry
        if short in HANDLE_CLASSES:
            documented[HANDLE_CLASSES[short]] = _documented(getattr(mod, HANDLE_CLASSES[short]))
    return {"modules": modules, "documented": documented}


if __name__ == "__main__":
    text = json.dumps(dump(), indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    else:
        sys.stdout.write(text)
