"""The consolidation preview (include/ks_engine.h: ks_consolidate_at) is exported and bound, carries
its constants and its 32-byte record, and rejects a NULL engine or a NULL buffer with KS_EINVAL before
anything else happens — no device is needed."""
import ctypes as C
import os
import re

import numpy as np

from kubesim_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ks_engine.h")


def _call(L, h, nodes, out, rows, cap, n_ev, n_rows, after=None, info=None, m=1):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))
    return L.ks_consolidate_at(h, 0, m, p(nodes), p(out), p(rows), cap, q(n_ev), q(n_rows), p(after), p(info))


def _bufs():
    return dict(nodes=np.zeros(1, np.int32), out=np.full(32, 0x5A, np.uint8), rows=np.full(40, 0x5A, np.uint8),
                n_ev=np.full(1, 77, np.int64), n_rows=np.full(1, 77, np.int64), after=np.full(4, 77, np.int64),
                info=np.full(_lib.KS_CONSOLIDATE_INFO, 77, np.int64))


def _untouched(b):
    return bool((b["out"] == 0x5A).all() and (b["rows"] == 0x5A).all() and
                all((b[f] == 77).all() for f in ("n_ev", "n_rows", "after", "info")))


def test_new_entry_is_exported_and_bound():
    L = _lib.load()
    assert "ks_consolidate_at" in _lib.EXPORTED_SYMBOLS
    assert L.ks_consolidate_at.restype is C.c_int
    assert len(L.ks_consolidate_at.argtypes) == 11


def test_constants_agree_with_the_header():
    assert _lib.KS_CONSOLIDATE_INFO == 6 and _lib.KS_ABI_VERSION == 2
    with open(HEADER) as f:
        text = f.read()
    for name in ("KS_CONSOLIDATE_INFO", "KS_DRAIN_MAX_PODS", "KS_PLACE_MAX_SHAPES", "KS_PLACE_MAX_PODS"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    m = re.search(r"enum \{ KS_CONSOLIDATE_BLOCKED = (\d), KS_CONSOLIDATE_REMOVED = (\d), KS_CONSOLIDATE_DESTINATION = (\d) \};", text)
    assert m and [int(x) for x in m.groups()] == [_lib.KS_CONSOLIDATE_BLOCKED, _lib.KS_CONSOLIDATE_REMOVED,
                                                  _lib.KS_CONSOLIDATE_DESTINATION] == [0, 1, 2]
    # the rounds' limit is the device's list length less one
    with open(os.path.join(os.path.dirname(HEADER), "..", "kubernetes-simulator_amd", "csrc", "ks_query.h")) as f:
        dev = f.read()
    m = re.search(r"#define\s+KS_PLACE_L\s+(\d+)", dev)
    assert m and "kConsMaxPods = kPlaceL - 1" in dev and _lib.KS_CONSOLIDATE_MAX_ROUND == int(m.group(1)) - 1


def test_consolidation_record_layout():
    from kubesim_amd.engine import CONSOLIDATION_DTYPE
    assert CONSOLIDATION_DTYPE.itemsize == _lib.KS_CONSOLIDATION_BYTES == 32
    names = ("node", "evicted", "outcome", "rows", "block_status", "pad", "first_row")
    assert CONSOLIDATION_DTYPE.names == names
    assert [CONSOLIDATION_DTYPE.fields[f][1] for f in names] == [0, 4, 8, 12, 16, 20, 24]
    # the header's struct, field by field
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"typedef struct \{([^}]*)\} ks_consolidation;", text)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for t, decl in re.findall(r"(int64_t|int32_t)\s+([\w,\s]+);", body):
        fields += [(t, n.strip()) for n in decl.split(",")]
    assert fields == [("int32_t", n) for n in names[:6]] + [("int64_t", "first_row")]
    sizes = {"int64_t": np.int64, "int32_t": np.int32}
    assert [(n, np.dtype(sizes[t])) for t, n in fields] == [(n, CONSOLIDATION_DTYPE.fields[n][0]) for n in names]


def test_null_engine_is_invalid_argument():
    L = _lib.load()
    b = _bufs()
    assert _call(L, None, b["nodes"], b["out"], b["rows"], 1, b["n_ev"], b["n_rows"], b["after"], b["info"]) == _lib.KS_EINVAL
    assert _untouched(b)


def test_null_buffers_are_invalid_argument():
    """The arguments are checked before the handle is read: a placeholder handle is never
    dereferenced when nodes, out, n_evicted or n_rows is NULL, rows_out is NULL with room asked for,
    or cap < 0."""
    L = _lib.load()
    handle = C.create_string_buffer(64)
    h = C.cast(handle, C.c_void_p)
    b = _bufs()
    ok = dict(nodes=b["nodes"], out=b["out"], rows=b["rows"], cap=1, n_ev=b["n_ev"], n_rows=b["n_rows"])
    for bad in (dict(nodes=None), dict(out=None), dict(n_ev=None), dict(n_rows=None), dict(rows=None), dict(cap=-1),
                dict(rows=None, cap=-1)):
        kw = dict(ok, **bad)
        assert _call(L, h, after=b["after"], info=b["info"], **kw) == _lib.KS_EINVAL, bad
    assert handle.raw == bytes(64)
    assert _untouched(b)


def test_engine_method_exists():
    import inspect
    from kubesim_amd.engine import Engine
    sig = inspect.signature(Engine.consolidate_at)
    assert list(sig.parameters) == ["self", "t", "nodes", "rows", "after"]
    assert sig.parameters["rows"].default is True and sig.parameters["after"].default is False
