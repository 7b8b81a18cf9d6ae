"""flame_update_gram / flame_update_gram_scratch_bytes / flame_update_gram_max_clients on the host:
the symbols resolve, the header and the export list still agree, the launch-branch table is
unchanged (the entry point stands outside it, as the update guard's do), every invalid call is
refused with a code and a message before any HIP call, and the scratch bound is monotone and at most
1 GiB.  Then the same validation under ASan + UBSan from a stand-alone C driver
(tests/abi_asan/gram_driver.c).  No GPU call."""
import ctypes
import os
import re
import shutil

import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def _header_functions():
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(flame_[a-z0-9_]+)\s*\(", hdr)))


def test_symbols_resolve_and_table_unchanged():
    N, L = _lib()
    for name in ("flame_update_gram", "flame_update_gram_scratch_bytes", "flame_update_gram_max_clients"):
        assert name in N.EXPORTS and hasattr(L, name)
    assert _header_functions() == sorted(N.EXPORTS)
    assert L.flame_update_gram.restype is ctypes.c_int
    assert L.flame_launch_branches() == 100
    assert not any("gram" in n for n in N.launch_branch_counts())
    assert L.flame_update_gram_max_clients() == 1024
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    assert "NeurIPS 2017" in hdr and "int flame_update_gram(" in hdr and "v_mfma_f64_16x16x4_f64" in hdr


def test_engine_reports_max_clients():
    from flame_amd import engine
    assert engine.gram_max_clients() == 1024


def test_scratch_bound_is_monotone_and_at_most_a_gibibyte():
    _, L = _lib()
    sb = L.flame_update_gram_scratch_bytes
    chunks = list(range(1, 70)) + [100, 511, 512, 513, 2047, 2048, 2049, 4096, 8191, 8192, 8193, 24415, 100000,
                                   1 << 24, (1 << 31) - 1]
    clients = list(range(1, 131)) + [191, 192, 193, 256, 511, 512, 513, 1000, 1023, 1024]
    table = [[sb(c, n) for n in clients] for c in chunks]
    for row in table:
        assert all(0 < b <= GIB for b in row)
        assert all(a <= b for a, b in zip(row, row[1:]))                     # in n_clients
    for lo, hi in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(lo, hi))                           # in n_chunks
    assert sb(24415, 1024) <= GIB
    assert sb(0, 9) == 0 and sb(-3, 9) == 0 and sb(5, 0) == 0 and sb(5, 1025) == 0 and sb(1 << 31, 9) == 0


def test_gram_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    big = 1 << 40

    def call(dtype=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=9, gram=fake, nf=fake, scratch=fake,
             sbytes=big):
        return L.flame_update_gram(dtype, segs, n_segs, n_chunks, clients, n_clients, gram, nf, scratch, sbytes, None)
    err = L.flame_last_error
    assert call(segs=None) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=0) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=-1) == N.FLAME_EINVAL and b"segment" in err()
    assert call(clients=None) == N.FLAME_EINVAL and b"client pointer" in err()
    assert call(n_chunks=0) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=1 << 31) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_clients=0) == N.FLAME_EINVAL and b"n_clients" in err()
    assert call(n_clients=-3) == N.FLAME_EINVAL and b"n_clients" in err()
    assert call(n_clients=1025) == N.FLAME_ENOTSUP and b"1024" in err() and b"n_clients" in err()
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"float dtypes only" in err()
    assert call(dtype=21) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(dtype=-1) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(gram=None) == N.FLAME_EINVAL and b"output array" in err()
    assert call(nf=None) == N.FLAME_EINVAL and b"output array" in err()
    assert call(scratch=None) == N.FLAME_EINVAL and b"scratch" in err()
    need = L.flame_update_gram_scratch_bytes(1, 9)
    assert call(sbytes=need - 1) == N.FLAME_EINVAL and b"too small" in err() and str(need).encode() in err()
    assert call(sbytes=0) == N.FLAME_EINVAL and b"too small" in err()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_gram_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("gram_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "gram abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
