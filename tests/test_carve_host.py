"""The query scratch layouts of kubernetes-simulator_amd/csrc/ks_carve.h, compiled for the host
(tests/native/carve_host.cpp): at the edge counts of ks_place_at, ks_drain_at and the per-node lists
every carved range lies inside the reserved size, overlaps no other, is aligned for its element, and
sits at the offset the entry points' earlier hand-written formulas give.  No device is needed."""
import ctypes as C
import functools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "carve_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "ks_carve.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(CSRC, "ks_query.h")]


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostcarve.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    lb.ks_host_carve_check.restype = C.c_int64
    return lb


def test_every_layout_matches_its_reserved_size_and_the_earlier_offsets():
    assert host_lib().ks_host_carve_check() == 0
