"""The step plan and the profile accounting of kubernetes-simulator_amd/csrc/ks_plan.h, compiled for
the host (tests/native/plan_host.cpp): plan_step over every combination of its inputs against the
four booleans and the list-length rule ks_step's body held before, and batch_record / account_batch
for each chain at a pass's first, middle, last and only batch against the accounting by event index
and `kind` bits, every ks_kernel_stats field and the three ks_step_stats sums.  No device is needed."""
import ctypes as C
import functools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plan_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "ks_plan.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(HERE, "..", "include", "ks_engine.h")]


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostplan.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    lb.ks_host_plan_check.restype = C.c_int64
    lb.ks_host_account_check.restype = C.c_int64
    return lb


def test_plan_matches_the_earlier_booleans_on_every_combination():
    assert host_lib().ks_host_plan_check() == 0


def test_accounting_matches_the_earlier_formulas_on_every_chain_and_position():
    assert host_lib().ks_host_account_check() == 0
