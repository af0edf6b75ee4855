"""Merge over the C-ABI (``gs_merge_*`` in include/gpusort.h): two arrays this library sorted into one: keys, pairs or positions.

``a[0 .. na)`` and ``b[0 .. nb)`` are sorted ascending or descending under the library's total order of their key type (floats by the
order-preserving flip: ``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN``); the result is the STABLE merge: sorted in the same order,
and among keys with the same bits all of ``a``'s come before all of ``b``'s, each side in its input order: what a stable pairs sort of
``[a; b]`` gives, for one read and one write of every element.  Equality is BITWISE in that order: ``-0.0`` and ``+0.0`` are two keys and
every NaN pattern is a key of its own.  The order of the inputs is not checked: on unsorted inputs the output is unspecified, but every
output slot is written once, every position lies below ``na + nb`` and nothing outside the buffers is touched.  No counterpart in the
reference project.  PyTorch is used only for device memory and the current HIP stream, and is imported inside the functions that need
it.  The numpy statement of the semantics is ``merge_reference``.

Why this module is privately named: tests/test_python_api_cpu.py pins the public names of every module of the package to
tests/golden/python_api.json and lets a new module in only under a private name, so the whole Python layer of the family, its
``GS_MERGE_*`` constants included, lives here and is used as ``from gpusorting_amd._merge import merge, merge_by_key, argmerge, Merge``.
Moving it to ``gpusorting_amd.merge`` with package-level exports regenerates that fixture and is a follow-up.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle, _lib
from ._handle import (KEY32_TYPES, KEY64_TYPES, KEY_FLOAT32, KEY_FLOAT64, KEY_INT32, KEY_INT64, KEY_UINT32,  # noqa: F401
                      KEY_UINT64, ORDER_ASCENDING, ORDER_DESCENDING, _require_room, _stream_ptr)
from ._lib import check
from .segsort import sortable_bits
from .unique64 import sortable_bits64

# include/gpusort.h: the forms gs_merge_last reports, the plan and report words
GS_MERGE_FORM_NONE, GS_MERGE_FORM_KEYS, GS_MERGE_FORM_PAIRS, GS_MERGE_FORM_POSITIONS = 0, 1, 2, 3
(GS_MERGE_P_TILE, GS_MERGE_P_VT, GS_MERGE_P_THREADS, GS_MERGE_P_GRID, GS_MERGE_P_LDS_BYTES) = range(5)
GS_MERGE_PLAN_WORDS = 8
(GS_MERGE_R_FORM, GS_MERGE_R_NA, GS_MERGE_R_NB, GS_MERGE_R_TILES, GS_MERGE_R_COPY_TILES) = range(5)
GS_MERGE_R_PLAN = 8
GS_MERGE_REPORT_WORDS = 16
TILE = {4: 8192, 8: 4096}  # T by key width (GS_MG_TILE / GS_MG_TILE64 of merge_kernels.hpp)
THREADS = 512
_PLAN = ("tile", "vt", "threads", "grid", "lds_bytes")  # GS_MERGE_P_*
_REPORT = ("form", "na", "nb", "tiles", "copy_tiles")  # GS_MERGE_R_*


def _words(a: np.ndarray, key_type: int, descending: bool) -> np.ndarray:
    """The unsigned pattern whose ascending order is the declared order: the sortable bits, inverted for descending."""
    k = np.ascontiguousarray(a)
    if key_type in KEY32_TYPES:
        if k.dtype.itemsize != 4 or k.ndim != 1:
            raise ValueError("the 32-bit key types take 1-D arrays of 4-byte elements")
        w = sortable_bits(k, key_type)
    elif key_type in KEY64_TYPES:
        if k.dtype.itemsize != 8 or k.ndim != 1:
            raise ValueError("the 64-bit key types take 1-D arrays of 8-byte elements")
        w = sortable_bits64(k, key_type)
    else:
        raise ValueError("merge takes 32- and 64-bit keys (KEY_UINT32 .. KEY_FLOAT64)")
    return ~w if descending else w


def merge_reference(a: np.ndarray, b: np.ndarray, key_type: int = KEY_UINT32, descending: bool = False, a_values: np.ndarray | None = None,
                    b_values: np.ndarray | None = None):
    """What the ``gs_merge_*`` entries deliver: ``(keys, src)`` or, with values, ``(keys, src, values)``: the stable argsort of the words
    of the concatenation ``[a; b]`` (the sortable bits, inverted for descending), so that among equal words ``a``'s elements come first
    and both sides keep their order.  ``src`` is uint32: ``i`` for ``a[i]``, ``na + j`` for ``b[j]``.  ``a`` and ``b`` must be sorted in
    the declared order."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype:
        raise ValueError("one dtype for both sides")
    if (a_values is None) != (b_values is None):
        raise ValueError("values for both sides or for neither")
    src = np.argsort(np.concatenate([_words(a, key_type, descending), _words(b, key_type, descending)]), kind="stable")
    keys = np.concatenate([a, b])[src]
    if a_values is None:
        return keys, src.astype(np.uint32)
    a_values, b_values = np.ascontiguousarray(a_values), np.ascontiguousarray(b_values)
    if a_values.dtype != b_values.dtype or a_values.shape != a.shape or b_values.shape != b.shape:
        raise ValueError("one value per key, one dtype for both sides")
    return keys, src.astype(np.uint32), np.concatenate([a_values, b_values])[src]


def temp_bytes(max_keys: int, key_bytes: int = 4) -> int:
    """``gs_merge_temp_bytes`` (host only): the control block; 0 for invalid arguments."""
    return int(_lib.load().gs_merge_temp_bytes(int(max_keys), int(key_bytes)))


def merge_plan_reference(na: int, nb: int, key_bytes: int = 4) -> dict:
    """The Python statement of ``gs_merge_plan`` (tests compare the two word for word): T, VT, the threads, the grid and the LDS of
    the tile kernel."""
    n = int(na) + int(nb)
    if key_bytes not in (4, 8) or int(na) < 0 or int(nb) < 0 or not 0 < n <= _lib.GS_MAX_KEYS:
        raise ValueError("1 <= na + nb <= GS_MAX_KEYS; key_bytes 4 or 8")
    tile = TILE[key_bytes]
    return {"tile": tile, "vt": tile // THREADS, "threads": THREADS, "grid": -(-n // tile), "lds_bytes": tile * (key_bytes + 2) + 8}


def merge_plan(na: int, nb: int, key_bytes: int = 4) -> dict:
    """``gs_merge_plan`` (host only) by name: ``tile`` (T: outputs per workgroup), ``vt`` (outputs per thread), ``threads``, ``grid``
    (ceil((na + nb) / T)) and ``lds_bytes``."""
    plan = (C.c_uint32 * GS_MERGE_PLAN_WORDS)()
    check(_lib.load().gs_merge_plan(int(na), int(nb), int(key_bytes), plan), "gs_merge_plan")
    return {name: int(plan[i]) for i, name in enumerate(_PLAN)}


class Merge(_handle.Handle):
    """One ``gs_merge`` handle for merges of up to ``max_keys`` outputs (``na + nb``) of keys as wide as ``key_type``.

    The handle owns a 4 KiB control block and nothing that grows with the sizes; ``key_type`` and ``order`` are the defaults of its
    calls, and any key type of the same width and either order may be given per call.  No call waits on the host; one call is in flight
    per handle."""

    _PREFIX, _KEY_TYPES = "gs_merge_", KEY32_TYPES + KEY64_TYPES
    _KEYS_WANTED = "Merge takes 32- and 64-bit keys (KEY_UINT32 .. KEY_FLOAT64)"

    def __init__(self, max_keys: int, key_type: int = KEY_UINT32, order: int = ORDER_ASCENDING, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.order = int(max_keys), order
        self.key_bytes = 8 if self.key_type in KEY64_TYPES else 4
        self._create(device, self.max_keys, self.key_bytes)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.key_bytes))

    def _sides(self, a, b, na, nb):
        """``(na, nb, the side that names device and dtype)``: a side may be ``None`` or empty, not both."""
        na = (0 if a is None else a.numel()) if na is None else int(na)
        nb = (0 if b is None else b.numel()) if nb is None else int(nb)
        for t, n, name in ((a, na, "a"), (b, nb, "b")):
            if t is not None and t.element_size() != self.key_bytes:
                raise ValueError("%s must hold %d-byte elements" % (name, self.key_bytes))
            if n:
                _require_room(t, n, name)
                if t is None:
                    raise ValueError(f"{name} is None, n{name} = {n}")
        like = a if a is not None else b
        if like is None:
            raise ValueError("a and b are both None")
        return na, nb, like

    @staticmethod
    def _side_ptr(t, n: int):
        return t.data_ptr() if (t is not None and n) else None

    def _out(self, t, n: int, like, name: str, width: int | None = None, dtype=None):
        import torch
        if t is None:
            t = torch.empty(n, dtype=like.dtype if dtype is None else dtype, device=like.device)
        if t.element_size() != (self.key_bytes if width is None else width):
            raise ValueError("%s must hold %d-byte elements" % (name, self.key_bytes if width is None else width))
        _require_room(t, n, name)
        return t

    def merge(self, a, b, na: int | None = None, nb: int | None = None, out=None, stream=None, key_type: int | None = None,
              order: int | None = None):
        """``gs_merge_keys``: the stable merge of ``a[:na]`` and ``b[:nb]`` into ``out[:na + nb]`` (``out``, or a fresh tensor).  A side
        may be empty or ``None``, not both.  Neither input is written, nothing at or behind element ``na + nb`` of ``out`` is."""
        na, nb, like = self._sides(a, b, na, nb)
        out = self._out(out, na + nb, like, "out")
        self._call("keys", self._side_ptr(a, na), na, self._side_ptr(b, nb), nb, out.data_ptr(), self.key_type if key_type is None else key_type,
                   self.order if order is None else order, _stream_ptr(stream))
        return out

    def merge_pairs(self, a_keys, a_values, b_keys, b_values, na: int | None = None, nb: int | None = None, out_keys=None, out_values=None,
                    stream=None, key_type: int | None = None, order: int | None = None):
        """``gs_merge_pairs``: ``(out_keys, out_values)``: the stable merge with every value following its key.  The values of both
        sides hold elements of one width, 4 or 8 bytes."""
        na, nb, like = self._sides(a_keys, b_keys, na, nb)
        vlike = a_values if a_values is not None else b_values
        if vlike is None:
            raise ValueError("a_values and b_values are both None")
        vb = vlike.element_size()
        for t, n, name in ((a_values, na, "a_values"), (b_values, nb, "b_values")):
            if t is not None and t.element_size() != vb:
                raise ValueError("a_values and b_values must hold elements of one width")
            if n:
                _require_room(t, n, name)
                if t is None:
                    raise ValueError(f"{name} is None")
        out_keys = self._out(out_keys, na + nb, like, "out_keys")
        out_values = self._out(out_values, na + nb, vlike, "out_values", width=vb)
        self._call("pairs", self._side_ptr(a_keys, na), self._side_ptr(a_values, na), na, self._side_ptr(b_keys, nb), self._side_ptr(b_values, nb),
                   nb, out_keys.data_ptr(), out_values.data_ptr(), vb, self.key_type if key_type is None else key_type,
                   self.order if order is None else order, _stream_ptr(stream))
        return out_keys, out_values

    def merge_positions(self, a, b, na: int | None = None, nb: int | None = None, out_keys=None, out_src=None, stream=None,
                        key_type: int | None = None, order: int | None = None):
        """``gs_merge_positions``: ``(out_keys, out_src)``: the merged keys and, as an int32 tensor holding uint32 values, where each
        came from: ``i`` for ``a[i]``, ``na + j`` for ``b[j]``: the index into ``[a; b]`` through which any payload is gathered."""
        import torch
        na, nb, like = self._sides(a, b, na, nb)
        out_keys = self._out(out_keys, na + nb, like, "out_keys")
        out_src = self._out(out_src, na + nb, like, "out_src", width=4, dtype=torch.int32)
        self._call("positions", self._side_ptr(a, na), na, self._side_ptr(b, nb), nb, out_keys.data_ptr(), out_src.data_ptr(),
                   self.key_type if key_type is None else key_type, self.order if order is None else order, _stream_ptr(stream))
        return out_keys, out_src

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): form (GS_MERGE_FORM_*; NONE after a refused call), na, nb, tiles (the tile
        kernel's workgroups that ran), copy_tiles (those that lay wholly in one input), and ``plan``: the words of
        ``merge_plan(na, nb, key_bytes)``."""
        w = self._words("last", GS_MERGE_REPORT_WORDS, stream)
        return {**{name: w[i] for i, name in enumerate(_REPORT)}, "plan": {name: w[GS_MERGE_R_PLAN + i] for i, name in enumerate(_PLAN)}}


# ---- the tensor functions ------------------------------------------------------------------------------------------------------------
_merge_cache: dict = {}
_VALUE_DTYPES = ("int32", "uint32", "float32", "int64", "uint64", "float64")


def _handle_for(device, n: int, key_type: int) -> Merge:
    """One ``Merge`` handle per (device, stream, key width), by functional's one cache rule; order and key type go with each call."""
    from .functional import _cached, _cap, _on
    wide = key_type in KEY64_TYPES
    return _cached(_merge_cache, _on(device) + (wide,), {"max_keys": n},
                   lambda max_keys: Merge(_cap(max_keys), KEY_UINT64 if wide else KEY_UINT32, device=device.index))


def _check_sides(a, b, unsigned: bool, name: str) -> int:
    """The refusals of the tensor functions that need no device; the key type of the call."""
    import torch
    from .functional import _KEY16_TYPE, _KEY64_TYPE, _KEY_TYPE, _key_type
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
        raise TypeError(f"{name} takes two tensors")
    if a.dtype != b.dtype:
        raise TypeError(f"b is {b.dtype}, a {a.dtype}: one dtype for both sides")
    dt = a.dtype
    if dt in _KEY16_TYPE:
        raise TypeError(f"unsupported key dtype {dt}: {name} on 16-bit keys is a follow-up; it takes 32- and 64-bit keys")
    if dt not in _KEY_TYPE and dt not in _KEY64_TYPE:
        raise TypeError(f"unsupported key dtype {dt}: {name} takes 32- and 64-bit keys (int32, uint32, float32, int64, uint64, float64)")
    return _key_type(a, unsigned, _KEY_TYPE if dt in _KEY_TYPE else _KEY64_TYPE)


def _check_placed(*tensors) -> None:
    """Behind the dtype refusals: every tensor of the call 1-D, contiguous and on the first one's GPU."""
    first = tensors[0]
    if any(t.dim() != 1 or not t.is_contiguous() or t.device != first.device for t in tensors) or first.device.type != "cuda":
        raise ValueError("every tensor of the call must be a contiguous 1-D tensor on one GPU")


def merge(a, b, descending: bool = False, unsigned: bool = False):
    """The stable merge of two 1-D contiguous GPU tensors of one dtype, each sorted by this library ascending or ``descending``, as a
    new tensor of ``a.numel() + b.numel()`` elements: int32, float32, int64, float64 (uint32 / uint64 where torch has them;
    ``unsigned=True`` reads signed storage as unsigned keys); floats in the order ``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf <
    +NaN``, compared BITWISE.  Either side may be empty.  The order of the inputs is not checked.  No wait on the host.  16-bit dtypes
    are a ``TypeError``."""
    import torch
    from .functional import _order
    kt = _check_sides(a, b, unsigned, "merge")
    _check_placed(a, b)
    n = a.numel() + b.numel()
    if n == 0:
        return torch.empty(0, dtype=a.dtype, device=a.device)
    with torch.cuda.device(a.device):
        return _handle_for(a.device, n, kt).merge(a, b, key_type=kt, order=_order(descending))


def merge_by_key(a_keys, a_values, b_keys, b_values, descending: bool = False, unsigned: bool = False):
    """``(keys, values)``: ``merge`` of the keys with every value following its key: among equal keys ``a``'s pairs come first and
    both sides keep their order, as a stable pairs sort of the concatenation would leave them.  The values are 1-D contiguous tensors
    of one dtype (int32, uint32, float32, int64, uint64, float64), one per key."""
    import torch
    from .functional import _order
    kt = _check_sides(a_keys, b_keys, unsigned, "merge_by_key")
    if not isinstance(a_values, torch.Tensor) or not isinstance(b_values, torch.Tensor):
        raise TypeError("merge_by_key takes two value tensors")
    if a_values.dtype != b_values.dtype:
        raise TypeError(f"b_values are {b_values.dtype}, a_values {a_values.dtype}: one dtype for both sides")
    if a_values.dtype not in tuple(getattr(torch, d) for d in _VALUE_DTYPES if hasattr(torch, d)):
        raise TypeError(f"unsupported value dtype {a_values.dtype}: merge_by_key takes " + ", ".join(_VALUE_DTYPES))
    if a_values.shape != a_keys.shape or b_values.shape != b_keys.shape:
        raise ValueError("one value per key")
    _check_placed(a_keys, b_keys, a_values, b_values)
    n = a_keys.numel() + b_keys.numel()
    if n == 0:
        return torch.empty(0, dtype=a_keys.dtype, device=a_keys.device), torch.empty(0, dtype=a_values.dtype, device=a_keys.device)
    with torch.cuda.device(a_keys.device):
        return _handle_for(a_keys.device, n, kt).merge_pairs(a_keys, a_values, b_keys, b_values, key_type=kt, order=_order(descending))


def argmerge(a, b, descending: bool = False, unsigned: bool = False):
    """``(keys, src)``: ``merge`` and, as int32, where every element came from: ``i`` for ``a[i]``, ``a.numel() + j`` for ``b[j]``:
    ``torch.cat([a, b])[src]`` is ``keys``, and any payload stored beside ``[a; b]`` is gathered through ``src``."""
    import torch
    from .functional import _order
    kt = _check_sides(a, b, unsigned, "argmerge")
    _check_placed(a, b)
    n = a.numel() + b.numel()
    if n == 0:
        return torch.empty(0, dtype=a.dtype, device=a.device), torch.empty(0, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        return _handle_for(a.device, n, kt).merge_positions(a, b, key_type=kt, order=_order(descending))
