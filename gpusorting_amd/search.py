"""Sorted search over the C-ABI (``gs_search_*`` in include/gpusort.h): the lower / upper bound of many queries in an array this library
sorted: where each new key falls in the sorted keys a caller already has.

``hay[0 .. n)`` is sorted ascending or descending under the library's total order of its key type (floats by the order-preserving flip:
``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN``); ``out[j]`` is the number of haystack keys strictly in front of ``q[j]``
(left) or in front of or equal to it (right): the insertion position that keeps ``hay`` sorted.  Equality is BITWISE in that order:
``-0.0`` and ``+0.0`` are two keys and every NaN pattern is a key of its own, unlike ``torch.searchsorted``, which compares values and
knows ascending only.  The order of ``hay`` is not checked: on an unsorted haystack the positions are unspecified, but every one of them
lies in ``[0, n]`` and nothing outside the buffers is touched.  No counterpart in the reference project.  PyTorch is used only for device
memory and the current HIP stream.  The numpy statement of the semantics is ``searchsorted_reference``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle, _lib
from ._handle import KEY32_TYPES, KEY64_TYPES, _require_room, _stream_ptr
from ._lib import check
from .onesweep import KEY_FLOAT32, KEY_FLOAT64, KEY_INT32, KEY_INT64, KEY_UINT32, KEY_UINT64  # noqa: F401
from .segsort import sortable_bits
from .topk import ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401
from .unique64 import sortable_bits64

ROUTE_AUTO = ROUTE_NONE = 0
ROUTE_TILE, ROUTE_SORT, ROUTE_BINARY = 1, 2, 3
ROUTES = {"auto": ROUTE_AUTO, "tile": ROUTE_TILE, "sort": ROUTE_SORT, "binary": ROUTE_BINARY}
TABLE_AUTO, TABLE_ON, TABLE_OFF = 0, 1, 2
SAMPLE_BYTES, WINDOW_BYTES = 65536, 32768
_PLAN = ("tile", "window", "samples", "stride", "tile_grid", "binary_grid", "sample_grid", "table", "route_sorted", "route_unsorted",
         "route_no_engine")  # GS_SEARCH_P_*
_REPORT = ("route", "n", "m", "table", "lds_tiles", "global_tiles", "engine")  # GS_SEARCH_R_*


def _words(a: np.ndarray, key_type: int, descending: bool) -> np.ndarray:
    """The unsigned pattern whose ascending order is the declared order of the haystack: the sortable bits, inverted for descending."""
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
        raise ValueError("searchsorted takes 32- and 64-bit keys (KEY_UINT32 .. KEY_FLOAT64)")
    return ~w if descending else w


def searchsorted_reference(hay: np.ndarray, queries: np.ndarray, key_type: int = KEY_UINT32, descending: bool = False,
                           right: bool = False) -> np.ndarray:
    """What ``gs_search_sorted`` delivers: for every query the number of ``hay`` keys strictly in front of it in the declared order
    (``right=False``) or in front of or equal to it (``right=True``), as uint32: ``np.searchsorted`` on the flipped unsigned patterns,
    inverted for a descending haystack.  ``hay`` must be sorted in that order."""
    h, q = _words(hay, key_type, descending), _words(queries, key_type, descending)
    return np.searchsorted(h, q, side="right" if right else "left").astype(np.uint32)


def temp_bytes(max_keys: int, max_queries: int, key_bytes: int = 4, sort_queries: bool = False) -> int:
    """``gs_search_temp_bytes`` (host only); 0 for invalid arguments."""
    return int(_lib.load().gs_search_temp_bytes(int(max_keys), int(max_queries), int(key_bytes), 1 if sort_queries else 0))


def search_plan_reference(n: int, m: int, key_bytes: int = 4) -> dict:
    """The Python statement of ``gs_search_plan`` (tests compare the two word for word): T, W, the sample table, the grids, and the
    route AUTO takes."""
    n, m = int(n), int(m)
    if key_bytes not in (4, 8) or not (0 < n <= _lib.GS_MAX_KEYS and 0 < m <= _lib.GS_MAX_KEYS):
        raise ValueError("1 <= n, m <= GS_MAX_KEYS; key_bytes 4 or 8")
    cap = SAMPLE_BYTES // key_bytes
    stride = 1
    while -(-n // stride) > cap:
        stride *= 2
    tile, threads = 2048, 512
    table = m >= _lib.GS_SEARCH_TABLE_MIN_QUERIES
    sort = m >= _lib.GS_SEARCH_SORT_MIN_QUERIES and n >= _lib.GS_SEARCH_SORT_MIN_KEYS
    samples = n // stride
    return {"tile": tile, "window": WINDOW_BYTES // key_bytes, "samples": samples, "stride": stride, "tile_grid": -(-m // tile),
            "binary_grid": min(-(-m // threads), 512) if table else -(-m // 256), "sample_grid": -(-samples // 256), "table": int(table),
            "route_sorted": ROUTE_TILE, "route_unsorted": ROUTE_SORT if sort else ROUTE_BINARY, "route_no_engine": ROUTE_BINARY}


def search_plan(n: int, m: int, key_bytes: int = 4) -> dict:
    """``gs_search_plan`` (host only) by name: ``tile`` (T), ``window`` (W), ``samples``, ``stride`` (S), ``tile_grid``, ``binary_grid``,
    ``sample_grid``, ``table`` and AUTO's route for queries in order (``route_sorted``), in no order on a handle that sorts queries
    (``route_unsorted``) and on one that does not (``route_no_engine``)."""
    plan = (C.c_uint32 * _lib.GS_SEARCH_PLAN_WORDS)()
    check(_lib.load().gs_search_plan(int(n), int(m), int(key_bytes), plan), "gs_search_plan")
    return {name: int(plan[i]) for i, name in enumerate(_PLAN)}


class SortedSearch(_handle.Handle):
    """One ``gs_search`` handle for haystacks of up to ``max_keys`` keys and calls of up to ``max_queries`` queries of ``key_type``.

    ``sort_queries=True`` embeds the pairs sorter that route SORT needs (and its buffers: 2 x (key + 4) bytes per query); without it
    the handle holds 64 KiB and serves queries in order (TILE) and in any order one thread per query (BINARY).  ``search`` does not
    wait on the host."""

    _PREFIX, _KEY_TYPES = "gs_search_", KEY32_TYPES + KEY64_TYPES
    _KEYS_WANTED = "SortedSearch takes 32- and 64-bit keys (KEY_UINT32 .. KEY_FLOAT64)"

    def __init__(self, max_keys: int, max_queries: int, key_type: int = KEY_UINT32, order: int = ORDER_ASCENDING, sort_queries: bool = False,
                 device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.max_queries = int(max_keys), int(max_queries)
        self.order, self.sort_queries = order, bool(sort_queries)
        self.key_bytes = 8 if key_type in KEY64_TYPES else 4
        self._create(device, self.max_keys, self.max_queries, self.key_bytes, 1 if sort_queries else 0)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.max_queries, self.key_bytes, 1 if self.sort_queries else 0))

    def set_route(self, route) -> None:
        """``gs_search_set_route``: "auto", "tile", "sort", "binary" (or the ROUTE_* value) for the calls that follow."""
        self._call("set_route", ROUTES.get(route, route))

    def set_table(self, table: int) -> None:
        """``gs_search_set_table``: TABLE_AUTO, TABLE_ON or TABLE_OFF: the form of route BINARY."""
        self._call("set_table", int(table))

    def status(self, hay, queries, n: int | None = None, m: int | None = None, right: bool = False, queries_sorted: bool = False, out=None,
               stream=None, key_type: int | None = None, order: int | None = None):
        """``gs_search_sorted`` as ``(status code, out)``; ``search`` raises on a status other than GS_OK."""
        import torch
        if hay.element_size() != self.key_bytes or queries.element_size() != self.key_bytes:
            raise ValueError("hay and queries must hold %d-byte elements" % self.key_bytes)
        n = hay.numel() if n is None else int(n)
        m = queries.numel() if m is None else int(m)
        _require_room(hay, n, "hay")
        _require_room(queries, m, "queries")
        if out is None:
            out = torch.empty(m, dtype=torch.int32, device=queries.device)
        if out.element_size() != 4:
            raise ValueError("out must hold 4-byte elements")
        _require_room(out, m, "out")
        st = self._entry("sorted")(self._h, hay.data_ptr(), n, queries.data_ptr(), m, out.data_ptr(),
                                   self.key_type if key_type is None else key_type, self.order if order is None else order,
                                   _lib.GS_SEARCH_RIGHT if right else _lib.GS_SEARCH_LEFT, 1 if queries_sorted else 0, _stream_ptr(stream))
        return int(st), out

    def search(self, hay, queries, n: int | None = None, m: int | None = None, right: bool = False, queries_sorted: bool = False, out=None,
               stream=None):
        """``gs_search_sorted``: the positions of ``queries[:m]`` in ``hay[:n]`` as an int32 tensor holding uint32 values (``out``, or a
        fresh tensor of ``m`` elements).  ``queries_sorted=True`` declares the queries sorted in the haystack's order.  Neither input is
        written, nothing at or behind element ``m`` of ``out`` is."""
        st, out = self.status(hay, queries, n, m, right, queries_sorted, out, stream)
        check(st, "gs_search_sorted")
        return out

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, n, m, table, lds_tiles, global_tiles, engine, and ``plan``: the words of
        ``search_plan(n, m, key_bytes)``."""
        w = self._words("last", _lib.GS_SEARCH_REPORT_WORDS, stream)
        return {**{name: w[i] for i, name in enumerate(_REPORT)}, "plan": {name: w[_lib.GS_SEARCH_R_PLAN + i] for i, name in enumerate(_PLAN)}}
