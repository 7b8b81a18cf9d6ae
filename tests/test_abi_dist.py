"""flame_update_dist / flame_update_dist_scratch_bytes on the host: the symbols resolve, the header
and the export list still agree, the launch-branch table is unchanged (the entry point stands
outside it, as the statistics' does), every invalid call is refused with a code and a message
before any HIP call, and there is no client cap.  Then the same validation under ASan + UBSan from
a stand-alone C driver (tests/abi_asan/dist_driver.c).  No GPU call, and no sanitizer inside Python."""
import ctypes
import os
import re
import shutil

import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def _header_functions():
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(flame_[a-z0-9_]+)\s*\(", hdr)))


def test_symbols_resolve_and_table_unchanged():
    N, L = _lib()
    for name in ("flame_update_dist", "flame_update_dist_scratch_bytes"):
        assert name in N.EXPORTS and hasattr(L, name)
    assert _header_functions() == sorted(N.EXPORTS)
    assert L.flame_update_dist.restype is ctypes.c_int
    assert L.flame_update_dist.argtypes == L.flame_update_stats.argtypes
    assert L.flame_launch_branches() == 100
    assert not any("dist" in n for n in N.launch_branch_counts())
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    assert "Pillutla" in hdr and "IEEE Transactions" in hdr and "int flame_update_dist(" in hdr


def test_scratch_is_the_statistics_and_has_no_client_cap():
    _, L = _lib()
    sb, ref = L.flame_update_dist_scratch_bytes, L.flame_update_stats_scratch_bytes
    for c in (1, 7, 8, 9, 64, 4097, 24415, (1 << 31) - 1):
        for n in (1, 8, 9, 64, 65, 1024, 1025, 100000):
            assert sb(c, n) == ref(c, n) == -(-c // 8) * n * 8
    assert sb(0, 9) == 0 and sb(-3, 9) == 0 and sb(5, 0) == 0 and sb(5, -1) == 0 and sb(1 << 31, 9) == 0


def test_dist_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    big = 1 << 40

    def call(dtype=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=9, dist2=fake, nf=fake, scratch=fake,
             sbytes=big):
        return L.flame_update_dist(dtype, segs, n_segs, n_chunks, clients, n_clients, dist2, nf, scratch, sbytes, None)
    err = L.flame_last_error
    assert call(segs=None) == N.FLAME_EINVAL and b"segment" in err() and b"flame_update_dist" in err()
    assert call(n_segs=0) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=-1) == N.FLAME_EINVAL and b"segment" in err()
    assert call(clients=None) == N.FLAME_EINVAL and b"client pointer" in err()
    assert call(n_chunks=0) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=1 << 31) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_clients=0) == N.FLAME_EINVAL and b"n_clients" in err()
    assert call(n_clients=-3) == N.FLAME_EINVAL and b"n_clients" in err()
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"float dtypes only" in err() and b"flame_update_dist" in err()
    assert call(dtype=21) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(dtype=-1) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(dist2=None) == N.FLAME_EINVAL and b"output array" in err()
    assert call(nf=None) == N.FLAME_EINVAL and b"output array" in err()
    assert call(scratch=None) == N.FLAME_EINVAL and b"scratch" in err()
    need = L.flame_update_dist_scratch_bytes(1, 9)
    assert call(sbytes=need - 1) == N.FLAME_EINVAL and b"too small" in err() and str(need).encode() in err()
    assert call(sbytes=0) == N.FLAME_EINVAL and b"too small" in err()
    # 100,000 clients are no defect of their own: the refusal left is the scratch's
    assert call(n_clients=100000, sbytes=8) == N.FLAME_EINVAL and b"too small" in err() and b"800000" in err()
    # the statistics entry point keeps its own name in its messages
    assert L.flame_update_stats(0, None, 1, 1, fake, 9, fake, fake, fake, big, None) == N.FLAME_EINVAL
    assert b"flame_update_stats" in err()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_dist_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("dist_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "dist abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
