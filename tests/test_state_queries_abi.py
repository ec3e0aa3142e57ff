"""The past-tick state queries (include/ks_engine.h: ks_requested_at, ks_filter_at, ks_score_at,
ks_cluster_series, ks_node_peaks) reject a NULL engine or a NULL output with KS_EINVAL before
anything else happens — no device is needed."""
import ctypes as C

import numpy as np

from kubesim_amd import _lib

NEW = ("ks_requested_at", "ks_filter_at", "ks_score_at", "ks_cluster_series", "ks_node_peaks")


def _calls(L, eng, out):
    return {
        "ks_requested_at": lambda: L.ks_requested_at(eng, 0, out),
        "ks_filter_at": lambda: L.ks_filter_at(eng, 0, out),
        "ks_score_at": lambda: L.ks_score_at(eng, 0, out),
        "ks_cluster_series": lambda: L.ks_cluster_series(eng, 0, 1, out),
        "ks_node_peaks": lambda: L.ks_node_peaks(eng, 0, 1, out),
    }


def test_new_entries_are_exported_and_bound():
    L = _lib.load()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert getattr(L, sym).restype is C.c_int
    assert _lib.KS_SERIES_COLS == 7


def test_null_engine_is_invalid_argument():
    L = _lib.load()
    out = np.zeros(64, np.int64)
    for sym, call in _calls(L, None, out.ctypes.data_as(C.c_void_p)).items():
        assert call() == _lib.KS_EINVAL, sym
    assert not out.any()


def test_null_output_is_invalid_argument():
    """The arguments are checked before the handle is read: a placeholder handle is never
    dereferenced when the output pointer is NULL."""
    L = _lib.load()
    handle = C.create_string_buffer(64)
    for sym, call in _calls(L, C.cast(handle, C.c_void_p), None).items():
        assert call() == _lib.KS_EINVAL, sym
    assert handle.raw == bytes(64)


def test_engine_methods_exist():
    from kubesim_amd.engine import Engine
    for name in ("requested_at", "filter_at", "score_at", "cluster_series", "node_peaks"):
        assert callable(getattr(Engine, name))
