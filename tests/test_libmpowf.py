"""CPU: the text of art_amd/csrc/libmpowf.h (powf with glibc's steps, the per-pixel powf of PQ / PQ_inv outside their tables) compiled for the
host and held to the host's powf, bit for bit: the four exponents of PQ / PQ_inv over every kind of argument.  A NaN is a NaN whatever its
payload.  The GPU side of the claim is tests/test_gpu_tool_domains.py (Jzazbz colour correction on `negzero`, `huge`, `mixed_zeros`)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "libmpowf_host.cc")
HDR = os.path.join(os.path.dirname(HERE), "art_amd", "csrc", "libmpowf.h")
SO = os.path.join(HERE, "emul", "liblibmpowf_host.so")
EXPONENTS = (0.1593017578125, 134.034375, 7.460772656268214e-03, 6.277394636015326)       # color.cc:70-83
_fp = C.POINTER(C.c_float)


def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC])
    return C.CDLL(SO)


def arguments():
    rng = np.random.default_rng(11)
    n = 500000
    parts = [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32),              # every bit pattern
             rng.integers(0, 0x7f800001, n, dtype=np.uint64).astype(np.uint32).view(np.float32),           # every non-negative float
             rng.integers(0, 0x01000000, n, dtype=np.uint64).astype(np.uint32).view(np.float32),           # zero, subnormals, the smallest normals
             (0.5 + 2.5 * rng.random(n)).astype(np.float32),                                               # around 1
             (1.0 + 0.02 * rng.random(n)).astype(np.float32),                                              # PQ_inv's XX up to its pole at 1.00878
             np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0 ** -149, 2.0 ** -126, 3.4028235e38, 1e-10, 1e-14], np.float32)]
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.parametrize("y", EXPONENTS)
def test_the_headers_powf_is_the_hosts(y):
    x = arguments()
    mine, host = np.empty_like(x), np.empty_like(x)
    lib().pw_ref_powf(x.ctypes.data_as(_fp), C.c_float(y), mine.ctypes.data_as(_fp), host.ctypes.data_as(_fp), C.c_longlong(x.size))
    bad = (mine.view(np.uint32) != host.view(np.uint32)) & ~(np.isnan(mine) & np.isnan(host))
    print(f"y = {y!r}: {int(bad.sum())} of {x.size} results differ from the host's powf")
    assert not bad.any(), [(float(x[i]).hex(), float(mine[i]).hex(), float(host[i]).hex()) for i in np.argwhere(bad)[:5, 0]]
    assert np.isfinite(host).mean() > 0.5 and (host == 0).any() and np.isinf(host).any() and np.isnan(host).any()       # every arm is entered
