"""The scale-up preview (include/ks_engine.h: ks_scale_up_at) is exported and bound, carries its
constants and its 56- and 32-byte records, and rejects a NULL engine or a NULL buffer with KS_EINVAL
before anything else happens — no device is needed."""
import ctypes as C
import os
import re

import numpy as np

from kubesim_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ks_engine.h")
ARGS = ("req", "keymask", "tol", "sel", "shape_of", "options", "out", "rows", "info")


def _bufs():
    return dict(req=np.array([[1000, 1 << 30, 0]], np.int64), keymask=np.array([3], np.uint8), tol=np.zeros(1, np.uint64),
                sel=np.zeros(1, np.uint64), shape_of=np.zeros(1, np.int32), options=np.zeros(56, np.uint8),
                out=np.full(32, 0x5A, np.uint8), rows=np.full(24, 0x5A, np.uint8),
                info=np.full(_lib.KS_SCALEUP_INFO, 77, np.int64))


def _call(L, h, b, **null):
    p = lambda name: None if null.get(name) else b[name].ctypes.data_as(C.c_void_p)
    return L.ks_scale_up_at(h, 0, 1, p("req"), p("keymask"), p("tol"), p("sel"), 1, p("shape_of"), 1, p("options"), p("out"),
                            p("rows"), p("info"))


def _untouched(b):
    return bool((b["out"] == 0x5A).all() and (b["rows"] == 0x5A).all() and (b["info"] == 77).all())


def test_new_entry_is_exported_and_bound():
    L = _lib.load()
    assert "ks_scale_up_at" in _lib.EXPORTED_SYMBOLS
    assert L.ks_scale_up_at.restype is C.c_int
    assert len(L.ks_scale_up_at.argtypes) == 14


def test_constants_agree_with_the_header():
    assert (_lib.KS_SCALEUP_MAX_OPTIONS, _lib.KS_SCALEUP_MAX_NODES, _lib.KS_SCALEUP_INFO) == (64, 65536, 4)
    assert _lib.KS_ABI_VERSION == 2
    with open(HEADER) as f:
        text = f.read()
    for name in ("KS_SCALEUP_MAX_OPTIONS", "KS_SCALEUP_MAX_NODES", "KS_SCALEUP_INFO", "KS_PLACE_MAX_PODS", "KS_ABI_VERSION"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    with open(os.path.join(os.path.dirname(HEADER), "..", "kubernetes-simulator_amd", "csrc", "ks_query.h")) as f:
        dev = f.read()
    assert "kScaleMaxOptions = 64;" in dev and "kScaleMaxNodes = 65536;" in dev


def _header_fields(text, name):
    m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for t, decl in re.findall(r"(int64_t|uint64_t|int32_t)\s+([\w,\s\[\]]+);", body):
        fields += [(t, n.strip()) for n in decl.split(",")]
    return fields


def test_record_layouts():
    from kubesim_amd.engine import SCALE_OPTION_DTYPE, SCALE_RESULT_DTYPE
    with open(HEADER) as f:
        text = f.read()
    assert SCALE_OPTION_DTYPE.itemsize == 56 and SCALE_RESULT_DTYPE.itemsize == 32
    assert _header_fields(text, "ks_scale_option") == [("int64_t", "alloc[4]"), ("uint64_t", "taint"), ("uint64_t", "label"),
                                                       ("int32_t", "max_nodes"), ("int32_t", "pad")]
    assert SCALE_OPTION_DTYPE.names == ("alloc", "taint", "label", "max_nodes", "pad")
    assert [SCALE_OPTION_DTYPE.fields[f][1] for f in SCALE_OPTION_DTYPE.names] == [0, 32, 40, 48, 52]
    assert SCALE_OPTION_DTYPE.fields["alloc"][0] == np.dtype((np.int64, (4,)))
    names = ("ok", "over_capacity", "not_found", "on_new", "nodes_used", "first_unplaced", "path", "pad")
    assert _header_fields(text, "ks_scale_result") == [("int32_t", n) for n in names]
    assert SCALE_RESULT_DTYPE.names == names
    assert [SCALE_RESULT_DTYPE.fields[f][1] for f in names] == list(range(0, 32, 4))


def test_null_engine_is_invalid_argument():
    L = _lib.load()
    b = _bufs()
    assert _call(L, None, b) == _lib.KS_EINVAL
    assert _untouched(b)


def test_null_buffers_are_invalid_argument():
    """The arguments are checked before the handle is read: a placeholder handle is never
    dereferenced when req, keymask, tol, sel, options or out is NULL."""
    L = _lib.load()
    handle = C.create_string_buffer(64)
    h = C.cast(handle, C.c_void_p)
    b = _bufs()
    for name in ("req", "keymask", "tol", "sel", "options", "out"):
        assert _call(L, h, b, **{name: True}) == _lib.KS_EINVAL, name
    assert handle.raw == bytes(64)
    assert _untouched(b)


def test_engine_method_exists():
    from kubesim_amd.engine import Engine
    assert callable(getattr(Engine, "scale_up_at"))
