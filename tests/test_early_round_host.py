"""Where a pass takes the early read-back's snapshot (kubernetes-simulator_amd/csrc/ks_plan.h
early_round), compiled for the host (tests/native/early_round_host.cpp, as tests/test_plan_host.py
compiles its program).  For every chain: passes of 0, 1, min - 1, min, min + 1 and many rounds.  Only a
two-launch pass of at least the minimum takes a snapshot; it falls after a round that exists and is
followed by exactly early_k more, the last included.  No device is needed."""
import ctypes as C
import functools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "early_round_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "ks_plan.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(HERE, "..", "include", "ks_engine.h")]


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostearly.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    lb.ks_host_early_round.restype = C.c_int64
    lb.ks_host_early_round.argtypes = [C.c_int64, C.c_int]
    lb.ks_host_early_const.restype = C.c_int64
    lb.ks_host_early_const.argtypes = [C.c_int]
    return lb


def consts():
    lb = host_lib()
    return {n: lb.ks_host_early_const(i) for i, n in enumerate(("early_min", "early_k", "two_launch", "chains"))}


def test_the_early_read_back_takes_long_two_launch_passes_only():
    lb, c = host_lib(), consts()
    assert c["early_min"] > c["early_k"] + 1 and c["early_k"] >= 1
    for chain in range(c["chains"]):
        for rounds in (0, 1, c["early_min"] - 1, c["early_min"], c["early_min"] + 1, 171, 100_000):
            r = lb.ks_host_early_round(rounds, chain)
            if chain == c["two_launch"] and rounds >= c["early_min"]:
                assert r == rounds - 1 - c["early_k"] and 0 <= r < rounds - 1, (chain, rounds, r)
            else:
                assert r == -1, (chain, rounds, r)
