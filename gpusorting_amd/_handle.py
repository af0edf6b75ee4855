"""What every ctypes wrapper of a C-ABI handle family shares (``gs_<family>_*`` in include/gpusort.h): the construction frame, the
lifetime, ``status`` / ``check``, the rank mode, the report read-back and the lazily grown alternate buffers, each once; the tensor
predicates the wrappers call; and the mode / order / key-type constants, defined here and re-exported by the modules that always had them.

A family's wrapper states ``_PREFIX`` (its entries are ``_entry(name)`` = ``<_PREFIX><name>``), ``_KEY_TYPES`` and ``_KEYS_WANTED`` (the
text of its key-type refusal), mixes in what its C family has (``Checked``: a ``check`` entry; ``RankMode``: ``get_`` / ``set_rank_mode``;
``AltBuffers``: alternate key / value buffers of ``_ALT_DTYPE``), and writes its constructor (``_check_key_type``, its sizes,
``_create``), its calls and its report table.  DESIGN.md, "The Python wrappers", shows the shortest one.

``OneSweep`` and ``ShardedOneSweep`` (``create_ex``, borrowed handles, debug entries) stand on their own.  PyTorch is imported inside
the functions that need it, never with this module.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
KEY_UINT32, KEY_INT32, KEY_FLOAT32 = 0, 1, 2
KEY_UINT64, KEY_INT64, KEY_FLOAT64 = 3, 4, 5  # 8-byte keys: eight passes planned by one histogram sweep
KEY16_TYPES = (KEY_UINT16, KEY_INT16, KEY_FLOAT16, KEY_BFLOAT16)
KEY32_TYPES = (KEY_UINT32, KEY_INT32, KEY_FLOAT32)
KEY64_TYPES = (KEY_UINT64, KEY_INT64, KEY_FLOAT64)


def _stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _require_cuda(t, name: str) -> None:
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor on the GPU")


def _require_room(t, n: int, name: str) -> None:
    """The C-ABI takes raw pointers: every buffer handed over must hold at least n elements."""
    if t is not None:
        _require_cuda(t, name)
        if n > t.numel():
            raise ValueError(f"{name} holds {t.numel()} elements, n = {n}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _indexed(names) -> tuple:
    """A report table ``(name, index)`` for words that lie in the order of ``names``."""
    return tuple((name, i) for i, name in enumerate(names))


class Handle:
    """One C-ABI handle of the family ``_PREFIX``: ``self._h`` from ``<_PREFIX>create`` until ``close``."""

    _PREFIX = ""        # "gs_unique_": the family's entries are _PREFIX + name
    _KEY_TYPES = ()     # the key types the family takes; the first is the default where key_type=None is allowed
    _KEYS_WANTED = ""   # the ValueError text for any other key type

    def _entry(self, name: str):
        return getattr(self._lib, self._PREFIX + name)

    def _check_key_type(self, key_type):
        """The head of every constructor: a GPU is there and the key type is one of the family's (``None``: its first)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type is None:
            key_type = self._KEY_TYPES[0]
        if key_type not in self._KEY_TYPES:
            raise ValueError(self._KEYS_WANTED)
        return key_type

    def _pairs_mode(self, order: int, mode: int, value_bytes: int) -> None:
        """``order``, ``mode`` and ``value_bytes`` of a handle built with a MODE_*: pairs default to 4-byte values."""
        self.order, self.mode = order, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0

    def _create(self, device, *sizes) -> None:
        """The tail of every constructor: the library, the device, and ``<_PREFIX>create(&h, *sizes)``."""
        import torch
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p()
        check(self._entry("create")(C.byref(h), *sizes), self._PREFIX + "create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name: str, *args, where: str | None = None) -> None:
        """``<_PREFIX><name>(h, *args)``; a status other than GS_OK raises ``GpuSortError`` naming ``<_PREFIX><where or name>``."""
        check(self._entry(name)(self._h, *args), self._PREFIX + (where or name))

    def _words(self, name: str, words: int, stream=None) -> list:
        """The ``words`` report words that ``<_PREFIX><name>`` delivers (synchronises)."""
        buf = (C.c_uint32 * words)()
        self._call(name, buf, words, _stream_ptr(stream))
        return [int(x) for x in buf]

    def _report(self, name: str, words: int, table, stream=None) -> dict:
        """``_words`` named by ``table``: ``(name, index)`` pairs."""
        w = self._words(name, words, stream)
        return {key: w[i] for key, i in table}


class Checked:
    """For a family with a ``check`` entry."""

    def status(self, stream=None) -> int:
        """The family's ``check`` entry as a status code (synchronises): GS_OK, or what the last call ran into (GS_ERR_ARG: bad
        arguments on the device, such as offsets; GS_ERR_SIZE: a broken promise; GS_ERR_HIP ...)."""
        return int(self._entry("check")(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), self._PREFIX + "check")


class RankMode:
    """For a family with ``get_rank_mode`` / ``set_rank_mode``: the ranking inside a tile (0 ballot multi-split, 1 returning LDS atomic)."""

    @property
    def rank_mode(self) -> int:
        return int(self._entry("get_rank_mode")(self._h))

    def set_rank_mode(self, mode: int) -> None:
        """The family's ``set_rank_mode``, with no call in flight."""
        self._call("set_rank_mode", int(mode))


class AltBuffers:
    """For a family whose calls take alternate key / value buffers: grown lazily to the largest call, never shrunk."""

    _ALT_DTYPE = "int32"  # the torch dtype of the alternate keys: "int16" for 2-byte keys
    _alt_keys = _alt_vals = None

    def _alt(self, n: int):
        """``(alt_keys, alt_values | None)`` as pointers, each of at least ``n`` elements (values: of ``value_bytes``, if any)."""
        import torch
        if self._alt_keys is None or self._alt_keys.numel() < n:
            self._alt_keys = torch.empty(max(n, 1), dtype=getattr(torch, self._ALT_DTYPE), device=self.device)
        if self.value_bytes == 0:
            return self._alt_keys.data_ptr(), None
        if self._alt_vals is None or self._alt_vals.numel() < n:
            self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
        return self._alt_keys.data_ptr(), self._alt_vals.data_ptr()
