"""The headroom queries (include/ks_engine.h: ks_headroom_at, ks_headroom_series) are exported and
bound, carry their constants, and reject a NULL engine or a NULL buffer with KS_EINVAL before
anything else happens — no device is needed."""
import ctypes as C
import os
import re

import numpy as np

from kubesim_amd import _lib

NEW = ("ks_headroom_at", "ks_headroom_series")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ks_engine.h")


def _bufs():
    req = np.array([[1000, 1 << 30, 0]], np.int64)
    km = np.array([3], np.uint8)
    tol = np.zeros(1, np.uint64)
    sel = np.zeros(1, np.uint64)
    out = np.zeros(64, np.int64)
    return [req, km, tol, sel, out]


def _ptrs(bufs, null=None):
    return [None if i == null else b.ctypes.data_as(C.c_void_p) for i, b in enumerate(bufs)]


def test_new_entries_are_exported_and_bound():
    L = _lib.load()
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert getattr(L, sym).restype is C.c_int
    assert len(L.ks_headroom_at.argtypes) == 9
    assert len(L.ks_headroom_series.argtypes) == 9


def test_constants_agree_with_the_header():
    assert _lib.KS_HEADROOM_COLS == 9
    assert _lib.KS_HEADROOM_MAX_SHAPES == 64
    assert _lib.KS_HEADROOM_NODE_MAX == 2**31 - 1
    assert _lib.KS_ABI_VERSION == 2
    with open(HEADER) as f:
        text = f.read()
    for name in ("KS_HEADROOM_COLS", "KS_HEADROOM_MAX_SHAPES", "KS_HEADROOM_NODE_MAX", "KS_ABI_VERSION"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name


def test_null_engine_is_invalid_argument():
    L = _lib.load()
    bufs = _bufs()
    req, km, tol, sel, out = _ptrs(bufs)
    assert L.ks_headroom_at(None, 0, 1, req, km, tol, sel, out, None) == _lib.KS_EINVAL
    assert L.ks_headroom_series(None, 0, 1, 1, req, km, tol, sel, out) == _lib.KS_EINVAL
    assert not bufs[4].any()


def test_null_buffers_are_invalid_argument():
    """The arguments are checked before the handle is read: a placeholder handle is never
    dereferenced when a buffer is NULL."""
    L = _lib.load()
    handle = C.create_string_buffer(64)
    h = C.cast(handle, C.c_void_p)
    bufs = _bufs()
    for null in range(5):
        req, km, tol, sel, out = _ptrs(bufs, null)
        assert L.ks_headroom_at(h, 0, 1, req, km, tol, sel, out, None) == _lib.KS_EINVAL, null
        assert L.ks_headroom_series(h, 0, 1, 1, req, km, tol, sel, out) == _lib.KS_EINVAL, null
    assert handle.raw == bytes(64)
    assert not bufs[4].any()


def test_engine_methods_exist():
    from kubesim_amd.engine import Engine
    for name in ("headroom_at", "headroom_series"):
        assert callable(getattr(Engine, name))
