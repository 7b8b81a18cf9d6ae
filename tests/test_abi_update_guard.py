"""The update guard's entry points (flame_update_stats, flame_update_stats_scratch_bytes,
flame_agg_reduce_scaled) on the host: the symbols resolve, every invalid call is refused with a
code and a message before any HIP call, the launch-branch table is unchanged (the two entry points
stand outside it), and engine.plan carries the clip scales as it carries the rates.  Then the same
validation under ASan + UBSan from a stand-alone C driver (tests/abi_asan/guard_driver.c).  No GPU call."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbols_resolve_and_table_unchanged():
    N, L = _lib()
    assert L.flame_abi_version() == 1
    for name in ("flame_update_stats", "flame_update_stats_scratch_bytes", "flame_agg_reduce_scaled"):
        assert name in N.EXPORTS and hasattr(L, name)
    assert L.flame_update_stats.restype is ctypes.c_int and L.flame_agg_reduce_scaled.restype is ctypes.c_int
    assert L.flame_launch_branches() == 100
    names = list(N.launch_branch_counts())
    assert not any("update_stats" in n or "scaled" in n for n in names)
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    assert "differential_privacy.py:68-76" in hdr and "differential_privacy.py:79-82" in hdr


def test_scratch_bytes():
    N, L = _lib()
    f = L.flame_update_stats_scratch_bytes
    assert f(0, 9) == 0 and f(10, 0) == 0 and f(-1, -1) == 0 and f(1 << 31, 4) == 0
    assert f(1, 1) == 8
    # ceil(n_chunks / R) x n_clients doubles, R chunks per workgroup; monotone in both
    r = [f(c, 1) // 8 for c in range(1, 200)]
    assert all(b - a in (0, 1) for a, b in zip(r, r[1:])) and r[-1] > 1
    R = next(c for c in range(1, 200) if f(c + 1, 1) == 16)
    assert f(24415, 1024) == -(-24415 // R) * 1024 * 8
    # below 1 % of the bytes read at config 3's shape (1,024 x 25M fp32: 24,415 chunks of 4 KiB per client)
    assert f(24415, 1024) * 100 < 1024 * 25_000_000 * 4


def test_update_stats_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    need = L.flame_update_stats_scratch_bytes(100, 9)

    def call(dtype=0, segs=fake, n_segs=1, n_chunks=100, clients=fake, n_clients=9, sumsq=fake, nonfinite=fake,
             scratch=fake, sbytes=need):
        return L.flame_update_stats(dtype, segs, n_segs, n_chunks, clients, n_clients, sumsq, nonfinite, scratch,
                                    sbytes, None)
    err = L.flame_last_error
    assert call(segs=None) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=0) == N.FLAME_EINVAL
    assert call(n_chunks=0) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_clients=0) == N.FLAME_EINVAL and b"n_clients" in err()
    assert call(n_clients=-2) == N.FLAME_EINVAL
    assert call(clients=None) == N.FLAME_EINVAL and b"client pointer" in err()
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"integer" in err()
    assert call(dtype=17) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(dtype=-1) == N.FLAME_ENOTSUP
    assert call(sumsq=None) == N.FLAME_EINVAL and b"output" in err()
    assert call(nonfinite=None) == N.FLAME_EINVAL and b"output" in err()
    assert call(scratch=None) == N.FLAME_EINVAL and b"scratch" in err()
    assert call(sbytes=need - 1) == N.FLAME_EINVAL and b"too small" in err()
    assert str(need - 1).encode() in err() and str(need).encode() in err()       # both sizes in the message


def test_reduce_scaled_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)

    def call(dtype=0, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=1, r32=fake, r64=fake,
             s32=fake, s64=fake):
        return L.flame_agg_reduce_scaled(dtype, flags, segs, n_segs, n_chunks, clients, n_clients, r32, r64, s32, s64,
                                         None)
    err = L.flame_last_error
    assert call(segs=None, n_segs=0) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_chunks=0) == N.FLAME_EINVAL
    assert call(clients=None) == N.FLAME_EINVAL and b"client pointer" in err()
    assert call(flags=N.FLAME_AGG_SEG_RATES) == N.FLAME_ENOTSUP and b"SEG_RATES" in err()
    assert call(flags=8) == N.FLAME_EINVAL and b"unknown flags" in err()
    assert call(flags=N.FLAME_AGG_INIT_FIRST, clients=None, n_clients=0) == N.FLAME_EINVAL
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"float dtypes only" in err()
    assert call(dtype=33) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(r32=None) == N.FLAME_EINVAL and b"rate" in err()
    assert call(dtype=N.FLAME_F64, r64=None) == N.FLAME_EINVAL and b"rate" in err()
    assert call(s32=None) == N.FLAME_EINVAL and b"scale" in err()
    assert call(dtype=N.FLAME_F64, s64=None) == N.FLAME_EINVAL and b"scale" in err()
    assert call(dtype=N.FLAME_F64, r32=None, s32=None, n_chunks=0) == N.FLAME_EINVAL   # f64 needs neither fp32 array


def test_plan_carries_scales_like_rates():
    from flame_amd import engine
    N, _ = _lib()
    seg = engine.Seg(100, out=4096, inp=4096, clients=[8192, 12288, 16384])
    scales = [1.0, 4.0 / (7.3 + 1e-6), 1e-41]
    p = engine.plan(N.FLAME_F32, [seg], [0.5, 0.25, 0.25], scales=scales)
    s32 = p.meta.view(np.float32)[p.off_s32 // 4: p.off_s32 // 4 + 3]
    s64 = p.meta.view(np.float64)[p.off_s64 // 8: p.off_s64 // 8 + 3]
    assert list(s64) == scales                                        # handed over as fp64 ...
    assert list(s32) == [np.float32(s) for s in scales]               # ... rounded to fp32 (RNE) as rates are
    assert p.off_s32 % 8 == 0 and p.off_s64 % 8 == 0 and p.off_s64 + 24 == p.meta.nbytes
    q = engine.plan(N.FLAME_F32, [seg], [0.5, 0.25, 0.25])
    assert q.off_s32 == q.off_s64 == -1
    assert np.array_equal(q.meta, p.meta[:q.meta.size])               # without scales: the block as before
    with pytest.raises(ValueError):
        engine.plan(N.FLAME_F32, [seg], [0.5, 0.25, 0.25], scales=[1.0])
    with pytest.raises(ValueError):
        engine.plan(N.FLAME_F32, [seg], [0.5, 0.25, 0.25], scales=scales, compact=True)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_guard_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("guard_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "guard abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
