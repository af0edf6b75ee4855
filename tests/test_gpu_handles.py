"""GPU test of the frame the fifteen ctypes wrappers share (gpusorting_amd/_handle.py), every class at its smallest legal sizes
(max_keys 2^16, 16 segments, max_k 8, max_queries 2^16):

  * a fresh handle: where the class has them, ``status()`` is GS_OK and ``rank_mode`` is 0 or 1; ``temp_bytes``, where present, is what
    the module's ``temp_bytes(...)`` (or, in a module without one, the C entry) gives for the same sizes;
  * ``close()`` twice leaves ``_h is None`` and raises nothing;
  * a constructor call with ``max_keys = 0`` raises ``GpuSortError`` with GS_ERR_SIZE, named by the family's ``gs_<family>_create``, and
    the half-built object can be dropped, closed and ``__del__``-ed;
  * a key type of the wrong width raises the class's own ``ValueError`` text (recorded from the code before the classes shared a base).

Only refused arguments: no kernel is launched here."""
import importlib

import pytest

pytestmark = pytest.mark.gpu

KEYS, SEGS, K, QUERIES = 1 << 16, 16, 8, 1 << 16
U32, U64, U16 = 0, 3, 6  # KEY_UINT32, KEY_UINT64, KEY_UINT16

# module, class, sizes, create label, a key type of the wrong width, the refusal's text, module temp_bytes arguments (None: no such function)
CASES = [
    ("segsort", "SegmentedSort", dict(max_keys=KEYS, max_segments=SEGS), "gs_segsort_create", U16, "the segmented sort takes 32-bit keys only", None),
    ("segsort16", "SegmentedSort16", dict(max_keys=KEYS, max_segments=SEGS), "gs_segsort16_create", U32,
     "SegmentedSort16 takes 16-bit key types only", None),
    ("rowsort", "RowSort", dict(max_keys=KEYS), "gs_sort_rows_create", U16, "RowSort takes 32-bit key types only", None),
    ("rowsort16", "RowSort16", dict(max_keys=KEYS), "gs_sort_rows16_create", U32, "RowSort16 takes 16-bit key types only", None),
    ("sort16", "Sort16", dict(max_keys=KEYS), "gs_sort16_create", U32, "Sort16 takes 16-bit key types only", None),
    ("topk", "TopK", dict(max_keys=KEYS, max_k=K), "gs_topk_create", U64,
     "the selection takes 32-bit keys, and 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16) in select_rows", None),
    ("topk16", "TopK16", dict(max_keys=KEYS, max_k=K), "gs_topk16_create", U32,
     "TopK16 takes 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16); 32-bit keys go to TopK", (KEYS, K, 0, 0)),
    ("segtopk", "SegmentedTopK", dict(max_keys=KEYS, max_segments=SEGS, max_k=K), "gs_segtopk_create", U16,
     "SegmentedTopK takes 32-bit keys only", None),
    ("segtopk16", "SegmentedTopK16", dict(max_keys=KEYS, max_segments=SEGS, max_k=K), "gs_segtopk16_create", U32,
     "SegmentedTopK16 takes 16-bit keys only", None),
    ("unique", "Unique", dict(max_keys=KEYS), "gs_unique_create", U16, "Unique takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)", (KEYS, 0, 0)),
    ("unique16", "Unique16", dict(max_keys=KEYS), "gs_unique16_create", U32,
     "Unique16 takes 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16); 32-bit keys go to Unique", (KEYS,)),
    ("unique64", "Unique64", dict(max_keys=KEYS), "gs_unique64_create", U32, "Unique64 takes 64-bit keys (KEY_UINT64, KEY_INT64, KEY_FLOAT64)",
     (KEYS, 0, 0)),
    ("reduce", "ReduceByKey", dict(max_keys=KEYS), "gs_reduce_create", U16, "ReduceByKey takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)",
     (KEYS, 4)),
    ("reduce64", "ReduceByKey64", dict(max_keys=KEYS), "gs_reduce64_create", U32,
     "ReduceByKey64 takes 64-bit keys (KEY_UINT64, KEY_INT64, KEY_FLOAT64)", (KEYS, 4)),
    ("search", "SortedSearch", dict(max_keys=KEYS, max_queries=QUERIES), "gs_search_create", U16,
     "SortedSearch takes 32- and 64-bit keys (KEY_UINT32 .. KEY_FLOAT64)", (KEYS, QUERIES, 4, False)),
]
# temp_bytes of the classes whose module has no function of that name: the C entry with the handle's own sizes
C_TEMP_BYTES = {"TopK": ("gs_topk_temp_bytes", (KEYS, K, 0)), "SegmentedTopK": ("gs_segtopk_temp_bytes", (SEGS,)),
                "SegmentedTopK16": ("gs_segtopk16_temp_bytes", (SEGS,))}
HAS_RANK_MODE = {"RowSort", "RowSort16", "Sort16", "SegmentedSort16", "SegmentedTopK", "SegmentedTopK16"}


@pytest.fixture(params=CASES, ids=[c[1] for c in CASES])
def case(request, gpu):
    module, name, sizes, label, wrong, text, temp_args = request.param
    mod = importlib.import_module("gpusorting_amd." + module)
    return mod, getattr(mod, name), sizes, label, wrong, text, temp_args


def _half_built(exc, cls):
    """The object whose constructor raised ``exc``: the ``self`` of the innermost frame of ``cls`` on the traceback."""
    found, tb = None, exc.__traceback__
    while tb is not None:
        if isinstance(tb.tb_frame.f_locals.get("self"), cls):
            found = tb.tb_frame.f_locals["self"]
        tb = tb.tb_next
    return found


def test_fresh_handle(case):
    from gpusorting_amd import _lib
    mod, cls, sizes, _, _, _, temp_args = case
    h = cls(**sizes)
    try:
        assert h._h
        assert hasattr(h, "check") == (cls.__name__ != "SortedSearch")
        if hasattr(h, "check"):
            assert h.status() == _lib.GS_OK
            h.check()
        assert hasattr(cls, "rank_mode") == hasattr(cls, "set_rank_mode") == (cls.__name__ in HAS_RANK_MODE)
        if hasattr(cls, "rank_mode"):
            assert h.rank_mode in (0, 1)
        assert hasattr(cls, "temp_bytes") == (temp_args is not None or cls.__name__ in C_TEMP_BYTES)
        if temp_args is not None:
            assert h.temp_bytes == mod.temp_bytes(*temp_args) > 0
        elif cls.__name__ in C_TEMP_BYTES:
            entry, args = C_TEMP_BYTES[cls.__name__]
            assert h.temp_bytes == getattr(_lib.load(), entry)(*args) > 0
    finally:
        h.close()


def test_close_twice(case):
    _, cls, sizes, _, _, _, _ = case
    h = cls(**sizes)
    h.close()
    assert h._h is None
    h.close()
    assert h._h is None
    h.__del__()


def test_failed_create(case):
    from gpusorting_amd import GpuSortError, _lib
    _, cls, sizes, label, _, _, _ = case
    with pytest.raises(GpuSortError) as e:
        cls(**dict(sizes, max_keys=0))
    assert e.value.status == _lib.GS_ERR_SIZE
    assert str(e.value).startswith(label + ":")
    half = _half_built(e.value, cls)
    assert half is not None and getattr(half, "_h", None) is None
    half.__del__()
    half.close()
    del half, e


def test_wrong_key_type(case):
    _, cls, sizes, _, wrong, text, _ = case
    with pytest.raises(ValueError) as e:
        cls(**sizes, key_type=wrong)
    assert str(e.value) == text and type(e.value) is ValueError
    half = _half_built(e.value, cls)
    assert half is not None and not hasattr(half, "_h")
    half.__del__()
    half.close()
