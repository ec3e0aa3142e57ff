"""The resource owners and the build-then-commit helper of kubernetes-simulator_amd/csrc/ks_own.h,
compiled for the host over counting fakes (tests/native/own_host.cpp): every owner frees exactly once
(destructor, move, move-assignment over a live owner, reset, empty), and a bundle of five members
whose k-th allocation fails, for each k, leaves its slot empty with every member made released, after
which a successful build fills the slot.  No device is needed."""
import ctypes as C
import functools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "own_host.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc", "ks_own.h")]


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostown.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", lib, SRC],
                       check=True)
    lb = C.CDLL(lib)
    lb.ks_host_own_check.restype = C.c_int64
    lb.ks_host_build_check.restype = C.c_int64
    return lb


def test_every_owner_frees_exactly_once():
    assert host_lib().ks_host_own_check() == 0


def test_a_failed_build_leaves_the_slot_empty_and_releases_what_it_made():
    assert host_lib().ks_host_build_check() == 0
