"""flame_noise_fill on the host: the symbol resolves, the header and the export list still agree, the
launch-branch table and the ABI version are unchanged (the entry point stands outside the table, as
the statistics' and the synthetic fill's do), every invalid call is refused with a code and a message
before any HIP call -- and what lives in device memory (the starts) is refused by the planner.  Then
the same validation under ASan + UBSan from a stand-alone C driver (tests/abi_asan/noise_driver.c).  No GPU
call, and no sanitizer inside Python."""
import ctypes
import math
import os
import re
import shutil

import numpy as np
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


def test_symbol_resolves_and_table_unchanged():
    N, L = _lib()
    assert "flame_noise_fill" in N.EXPORTS and hasattr(L, "flame_noise_fill")
    assert _header_functions() == sorted(N.EXPORTS)
    assert L.flame_noise_fill.restype is ctypes.c_int and len(L.flame_noise_fill.argtypes) == 10
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert not any("noise" in n for n in N.launch_branch_counts())
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    assert "int flame_noise_fill(" in hdr
    assert "differential_privacy.py:55-61" in hdr and "Salmon" in hdr and "Philox4x32-10" in hdr and "Box-Muller" in hdr


def test_noise_fill_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host

    def call(dtype=0, segs=fake, n_segs=1, n_chunks=1, streams=fake, starts=fake, seed=7, rnd=0, std=1.0):
        return L.flame_noise_fill(dtype, segs, n_segs, n_chunks, streams, starts, seed, rnd, std, None)
    err = L.flame_last_error
    assert call(segs=None) == N.FLAME_EINVAL and b"segment" in err() and b"flame_noise_fill" in err()
    assert call(n_segs=0) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_segs=-1) == N.FLAME_EINVAL and b"segment" in err()
    assert call(n_chunks=0) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
    assert call(n_chunks=1 << 31) == N.FLAME_EINVAL and b"n_chunks" in err()
    for dt in (N.FLAME_I64, N.FLAME_I32):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"float dtypes only" in err() and b"flame_noise_fill" in err()
    for dt in (6, 9, 21, -1):
        assert call(dtype=dt) == N.FLAME_ENOTSUP and b"unknown dtype" in err()
    assert call(streams=None) == N.FLAME_EINVAL and b"streams / starts" in err()
    assert call(starts=None) == N.FLAME_EINVAL and b"streams / starts" in err()
    for dt in range(4):
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
            assert call(dtype=dt, std=bad) == N.FLAME_EINVAL and b"std" in err() and b"flame_noise_fill" in err()
    # an std past fp32 is refused where the std is rounded to fp32, and only there: with FLAME_F64 the
    # same call gets as far as the next defect
    for dt in (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16):
        assert call(dtype=dt, std=1e39) == N.FLAME_EINVAL and b"infinite fp32" in err()
        mid = float.fromhex("0x1.ffffffp127")                  # FLT_MAX + half an ulp: RNE rounds it to infinity
        assert call(dtype=dt, std=mid) == N.FLAME_EINVAL and b"infinite fp32" in err()
        assert call(dtype=dt, std=math.nextafter(mid, 0.0), starts=None) == N.FLAME_EINVAL and b"streams / starts" in err()
    assert call(dtype=N.FLAME_F64, std=1e39, starts=None) == N.FLAME_EINVAL and b"streams / starts" in err()


def test_the_planner_refuses_what_lives_in_device_memory():
    """The starts and streams arrays are device memory to the library; engine.plan_noise builds them and
    refuses a negative start (or one past 2^62), a stream outside 32 bits and ragged arrays."""
    from flame_amd import engine
    segs = [engine.Seg(5, out=4096), engine.Seg(0, out=0), engine.Seg(4100, out=8192 + 4)]
    meta, n_chunks, offs = engine.plan_noise(0, segs, [0, 3, 4], [0, 0, (1 << 34) - 6], chunk=1024)
    assert n_chunks == 1 + 0 + 5 and offs["segs"] == 0 and offs["streams"] == 240 and offs["starts"] == 256
    head = meta[:30].reshape(3, 10)
    assert list(head[:, 0]) == [4096, 0, 8196] and list(head[:, 6]) == [5, 0, 4100] and list(head[:, 7]) == [0, 1, 1]
    assert list(head[:, 8]) == [0, 0, 1]                       # FLAME_SEG_UNALIGNED from the out pointer alone
    assert list(meta[30:32].view(np.uint32)) == [0, 3, 4, 0] and list(meta[32:35]) == [0, 0, (1 << 34) - 6]
    for starts in ([0, -1, 0], [0, 0, -(1 << 40)], [0, 0, 1 << 62], [0, 0, 1.0], [0, True, 0]):
        with pytest.raises(ValueError, match="start"):
            engine.plan_noise(0, segs, [0, 1, 2], starts, chunk=1024)
    for streams in ([0, -1, 0], [0, 1 << 32, 0], [0, 0.5, 0]):
        with pytest.raises(ValueError, match="stream"):
            engine.plan_noise(0, segs, streams, [0, 0, 0], chunk=1024)
    with pytest.raises(ValueError):
        engine.plan_noise(0, segs, [0, 1], [0, 0, 0], chunk=1024)
    with pytest.raises(ValueError):
        engine.plan_noise(0, [], [], [], chunk=1024)
    for seed, rnd, std in ((-1, 0, 1.0), (1 << 64, 0, 1.0), (True, 0, 1.0), (1.5, 0, 1.0), (7, -1, 1.0), (7, 0, -1.0),
                           (7, 0, float("nan")), (7, 0, float("inf"))):
        with pytest.raises(ValueError):
            engine.check_noise_args(seed, rnd, std)
    assert engine.check_noise_args(7, (1 << 32) + 5, 2) == (7, 5, 2.0)      # the round is taken mod 2^32


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_noise_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("noise_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "noise abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
