"""The gang admission preview (include/ks_engine.h: ks_gang_at) is exported and bound, carries its
constants and its 32-byte record, and rejects a NULL engine or a NULL buffer with KS_EINVAL before
anything else happens — no device is needed.  (Every other argument error, on a live engine:
tests/test_gang_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np

from kubesim_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ks_engine.h")
ARGS = ("req", "keymask", "tol", "sel", "shape_of", "first", "min_ok", "out", "rows", "after", "info")


def _call(L, h, b, flags=0, **over):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    a = dict({f: b[f] for f in ARGS}, **over)
    return L.ks_gang_at(h, 0, 1, p(a["req"]), p(a["keymask"]), p(a["tol"]), p(a["sel"]), 2, p(a["shape_of"]), 1, p(a["first"]),
                        p(a["min_ok"]), flags, p(a["out"]), p(a["rows"]), p(a["after"]), p(a["info"]))


def _bufs():
    return dict(req=np.array([[100, 100, 0]], np.int64), keymask=np.array([3], np.uint8), tol=np.zeros(1, np.uint64),
                sel=np.zeros(1, np.uint64), shape_of=np.zeros(2, np.int32), first=np.array([0, 2], np.int32),
                min_ok=np.array([2], np.int32), out=np.full(32, 0x5A, np.uint8), rows=np.full(48, 0x5A, np.uint8),
                after=np.full(4, 77, np.int64), info=np.full(_lib.KS_GANG_INFO, 77, np.int64))


def _untouched(b):
    return bool((b["out"] == 0x5A).all() and (b["rows"] == 0x5A).all() and (b["after"] == 77).all() and (b["info"] == 77).all())


def test_new_entry_is_exported_and_bound():
    L = _lib.load()
    assert "ks_gang_at" in _lib.EXPORTED_SYMBOLS
    assert L.ks_gang_at.restype is C.c_int
    assert len(L.ks_gang_at.argtypes) == 17 and L.ks_gang_at.argtypes[12] is C.c_uint32


def test_constants_agree_with_the_header():
    assert _lib.KS_GANG_INFO == 6 and _lib.KS_ABI_VERSION == 2
    with open(HEADER) as f:
        text = f.read()
    for name in ("KS_GANG_INFO", "KS_GANG_MAX_GANGS", "KS_GANG_MAX_PODS", "KS_GANG_MAX_SHAPES", "KS_GANG_NOT_TRIED",
                 "KS_DRAIN_MAX_PODS", "KS_PLACE_MAX_SHAPES", "KS_PLACE_MAX_PODS"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert _lib.KS_GANG_MAX_PODS == _lib.KS_DRAIN_MAX_PODS and _lib.KS_GANG_NOT_TRIED not in (0, 1, _lib.KS_PLACE_NOT_FOUND)
    m = re.search(r"#define\s+KS_GANG_STRICT\s+(\d+)u", text)
    assert m and int(m.group(1)) == _lib.KS_GANG_STRICT == 1
    m = re.search(r"enum \{ KS_GANG_BLOCKED = (\d), KS_GANG_ADMITTED = (\d), KS_GANG_SKIPPED = (\d) \};", text)
    assert m and [int(x) for x in m.groups()] == [_lib.KS_GANG_BLOCKED, _lib.KS_GANG_ADMITTED, _lib.KS_GANG_SKIPPED] == [0, 1, 2]
    # the rounds' limit is the device's list length
    with open(os.path.join(os.path.dirname(HEADER), "..", "kubernetes-simulator_amd", "csrc", "ks_query.h")) as f:
        dev = f.read()
    m = re.search(r"#define\s+KS_PLACE_L\s+(\d+)", dev)
    assert m and "kGangMaxPods = kPlaceL;" in dev and _lib.KS_GANG_MAX_ROUND == int(m.group(1))


def test_gang_record_layout():
    from kubesim_amd.engine import GANG_DTYPE
    assert GANG_DTYPE.itemsize == _lib.KS_GANG_BYTES == 32
    names = ("first", "size", "outcome", "tried", "ok", "over_capacity", "not_found", "block_status")
    assert GANG_DTYPE.names == names
    assert [GANG_DTYPE.fields[f][1] for f in names] == [0, 4, 8, 12, 16, 20, 24, 28]
    # the header's struct, field by field
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"typedef struct \{([^}]*)\} ks_gang;", text)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for t, decl in re.findall(r"(int64_t|int32_t)\s+([\w,\s]+);", body):
        fields += [(t, n.strip()) for n in decl.split(",")]
    assert fields == [("int32_t", n) for n in names]
    assert all(GANG_DTYPE.fields[n][0] == np.dtype(np.int32) for n in names)


def test_null_engine_is_invalid_argument():
    L = _lib.load()
    b = _bufs()
    assert _call(L, None, b) == _lib.KS_EINVAL
    assert _untouched(b)


def test_null_buffers_are_invalid_argument():
    """The arguments are checked before the handle is read: a placeholder handle is never
    dereferenced when shape_of, first or out — or one of the shape arrays — is NULL."""
    L = _lib.load()
    handle = C.create_string_buffer(64)
    h = C.cast(handle, C.c_void_p)
    b = _bufs()
    for bad in ("shape_of", "first", "out", "req", "keymask", "tol", "sel"):
        assert _call(L, h, b, **{bad: None}) == _lib.KS_EINVAL, bad
        assert _call(L, h, b, flags=_lib.KS_GANG_STRICT, **{bad: None}) == _lib.KS_EINVAL, bad
    assert _call(L, None, b, shape_of=None, first=None, out=None) == _lib.KS_EINVAL
    assert handle.raw == bytes(64)
    assert _untouched(b)


def test_engine_method_exists():
    import inspect
    from kubesim_amd.engine import Engine
    sig = inspect.signature(Engine.gang_at)
    assert list(sig.parameters) == ["self", "t", "shapes", "shape_of", "first", "min_ok", "strict", "rows", "after"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["min_ok"] is None and d["strict"] is False and d["rows"] is True and d["after"] is False
