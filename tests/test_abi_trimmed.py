"""flame_agg_trimmed / flame_agg_trimmed_max_k on the host: the symbols resolve, the launch-branch
table is unchanged (the entry point stands outside it, as the update guard's two do), every
invalid call is refused with a code and a message before any HIP call.  Then the same validation
under ASan + UBSan from a stand-alone C driver (tests/abi_asan/trimmed_driver.c).  No GPU call."""
import ctypes
import os
import shutil

import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbols_resolve_and_table_unchanged():
    N, L = _lib()
    for name in ("flame_agg_trimmed", "flame_agg_trimmed_max_k"):
        assert name in N.EXPORTS and hasattr(L, name)
    assert L.flame_agg_trimmed.restype is ctypes.c_int
    assert L.flame_launch_branches() == 100
    assert not any("trimmed" in n for n in N.launch_branch_counts())
    assert L.flame_agg_trimmed_max_k() == 16
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    assert "ICML 2018" in hdr and "no counterpart" in hdr and "int flame_agg_trimmed(" in hdr


def test_engine_reports_max_k():
    from flame_amd import engine
    assert engine.trimmed_max_k() == 16


def test_trimmed_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host

    def call(dtype=0, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=9, k=2):
        return L.flame_agg_trimmed(dtype, flags, segs, n_segs, n_chunks, clients, n_clients, k, None)
    err = L.flame_last_error
    assert call(segs=None) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=0) == N.FLAME_EINVAL and b"segment" in err()
    assert call(clients=None) == N.FLAME_EINVAL and b"client pointer" in err()
    assert call(n_chunks=0) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(k=-1) == N.FLAME_EINVAL and b"trim_k" in err()
    assert call(k=17, n_clients=100) == N.FLAME_ENOTSUP and b"trim_k" in err() and b"16" in err()
    assert call(k=4, n_clients=8) == N.FLAME_EINVAL and b"2 * trim_k" in err()      # n == 2k: nothing kept
    assert call(k=4, n_clients=7) == N.FLAME_EINVAL and b"2 * trim_k" in err()
    assert call(k=0, n_clients=0) == N.FLAME_EINVAL and b"n_clients" in err()
    assert call(k=0, n_clients=-3) == N.FLAME_EINVAL
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"float dtypes only" in err()
    assert call(dtype=21) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(dtype=-1) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(flags=8) == N.FLAME_EINVAL and b"unknown flags" in err()
    assert call(flags=1 << 20) == N.FLAME_EINVAL and b"unknown flags" in err()
    assert call(flags=N.FLAME_AGG_SEG_RATES) == N.FLAME_ENOTSUP and b"SEG_RATES" in err()
    assert call(flags=N.FLAME_AGG_SEG_RATES | N.FLAME_AGG_INIT_FIRST) == N.FLAME_ENOTSUP


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_trimmed_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("trimmed_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "trimmed abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
