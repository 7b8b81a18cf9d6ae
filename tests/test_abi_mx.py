"""flame_agg_reduce_mx on the host: the symbol resolves, the header and the export list agree, the
launch-branch table and the ABI version are unchanged, every refusal comes with its code and a message
naming the entry point before any HIP call, and every older reduce entry point refuses the two new
element codes.  Then the same validation under ASan + UBSan from a stand-alone C driver
(tests/abi_asan/mx_driver.c, built by tests/abi_asan/mx_driver.mk).  No GPU call, and no sanitizer inside Python."""
import atexit
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"flame_agg_reduce_mx"


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbol_resolves_and_table_unchanged():
    N, L = _lib()
    assert "flame_agg_reduce_mx" in N.EXPORTS and hasattr(L, "flame_agg_reduce_mx")
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(flame_[a-z0-9_]+)\s*\(", bare))) == sorted(N.EXPORTS)
    assert "int flame_agg_reduce_mx(int client_dtype, int agg_dtype, unsigned flags," in hdr
    vp = ctypes.c_void_p
    assert L.flame_agg_reduce_mx.restype is ctypes.c_int
    assert L.flame_agg_reduce_mx.argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_uint, vp, ctypes.c_int32, ctypes.c_int64,
                                              vp, vp, ctypes.c_int32, vp, vp, vp]
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert not any("mx" in n.split("_") for n in N.launch_branch_counts())
    # the two codes are the next free ones (6 .. 9 belong to flame_elementwise) and the header's
    assert (N.FLAME_FP8_E4M3, N.FLAME_FP8_E5M2) == (10, 11) == (N.FLAME_BOOL + 1, N.FLAME_BOOL + 2)
    assert re.search(r"#define FLAME_FP8_E4M3 10\b", hdr) and re.search(r"#define FLAME_FP8_E5M2 11\b", hdr)
    # the chunk is the client dtype's: one 4,096-byte slab tile, 16 elements per lane
    assert L.flame_chunk_elems(N.FLAME_FP8_E4M3) == L.flame_chunk_elems(N.FLAME_FP8_E5M2) == 4096 == N.FLAME_TILE_BYTES
    # the header states the per-element contract, the equivalence and the refusals
    for text in ("f32(q_i[e]) * f32_e8m0(s_i[e / 32])", "one IEEE fp32 multiply, denormals kept",
                 "a NaN element or scale byte 255", "round_f32(x * scale_i)", "round_f32(x * rate_i)", "round_f32(acc + t)",
                 "bit for bit what", "flame_agg_reduce_scaled) gives for FLAME_F32 over the", "dequantized update",
                 "client_tile_stride must", "FLAME_AGG_INIT_FIRST is", "FLAME_AGG_SEG_RATES is FLAME_ENOTSUP",
                 "ANY alignment"):
        assert text in hdr, text


def test_mx_refuses_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    E4, E5, F = N.FLAME_FP8_E4M3, N.FLAME_FP8_E5M2, N.FLAME_F32

    def call(cd=E4, ad=F, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, bscales=fake, n_clients=3, rates=fake,
             scales=None):
        return L.flame_agg_reduce_mx(cd, ad, flags, segs, n_segs, n_chunks, clients, bscales, n_clients, rates, scales, None)
    err = L.flame_last_error
    # every pair but (e4m3 | e5m2, f32): FLAME_ENOTSUP naming both dtypes
    codes = (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64, N.FLAME_I64, N.FLAME_I32, N.FLAME_U8, N.FLAME_BOOL,
             E4, E5, 12, 21, -1)
    for cd, ad in itertools.product(codes, codes):
        if cd in (E4, E5) and ad == F:
            continue
        assert call(cd=cd, ad=ad) == N.FLAME_ENOTSUP, (cd, ad)
        assert WHO in err() and b"client dtype %d" % cd in err() and b"aggregate dtype %d" % ad in err(), err()
    for cd in (E4, E5):
        for sc in (None, fake):
            assert call(cd=cd, scales=sc, flags=N.FLAME_AGG_INIT_FIRST) == N.FLAME_ENOTSUP
            assert WHO in err() and b"INIT_FIRST" in err()
            assert call(cd=cd, scales=sc, flags=N.FLAME_AGG_INIT_FIRST | N.FLAME_AGG_XCD_MAP) == N.FLAME_ENOTSUP
            assert call(cd=cd, scales=sc, flags=N.FLAME_AGG_SEG_RATES) == N.FLAME_ENOTSUP
            assert WHO in err() and b"SEG_RATES" in err()
            assert call(cd=cd, scales=sc, flags=8) == N.FLAME_EINVAL and WHO in err() and b"unknown flags" in err()
            assert call(cd=cd, scales=sc, flags=1 << 20) == N.FLAME_EINVAL and b"unknown flags" in err()
            assert call(cd=cd, scales=sc, segs=None) == N.FLAME_EINVAL and WHO in err() and b"segment" in err()
            assert call(cd=cd, scales=sc, n_segs=0) == N.FLAME_EINVAL and WHO in err() and b"segment" in err()
            assert call(cd=cd, scales=sc, n_chunks=0) == N.FLAME_EINVAL and WHO in err() and b"n_chunks" in err()
            assert call(cd=cd, scales=sc, n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
            assert call(cd=cd, scales=sc, n_chunks=2 ** 31) == N.FLAME_EINVAL and b"n_chunks" in err()
            assert call(cd=cd, scales=sc, clients=None) == N.FLAME_EINVAL and WHO in err() and b"client pointer" in err()
            assert call(cd=cd, scales=sc, bscales=None) == N.FLAME_EINVAL and WHO in err() and b"block scale pointer" in err()
            assert call(cd=cd, scales=sc, n_clients=0) == N.FLAME_EINVAL and WHO in err() and b"n_clients" in err()
            assert call(cd=cd, scales=sc, n_clients=-3) == N.FLAME_EINVAL and b"n_clients" in err()
            assert call(cd=cd, scales=sc, rates=None) == N.FLAME_EINVAL and WHO in err() and b"rate array" in err()


def test_older_entry_points_refuse_the_new_codes():
    """As they refuse any unknown code: FLAME_ENOTSUP before a launch (the tables are fake addresses)."""
    N, L = _lib()
    fake = ctypes.c_void_p(4096)
    err = L.flame_last_error
    for code in (N.FLAME_FP8_E4M3, N.FLAME_FP8_E5M2):
        assert L.flame_agg_reduce(code, 0, fake, 1, 1, fake, 3, fake, fake, None) == N.FLAME_ENOTSUP
        assert b"unsupported dtype %d" % code in err()
        assert L.flame_agg_reduce_scaled(code, 0, fake, 1, 1, fake, 3, fake, fake, fake, fake, None) == N.FLAME_ENOTSUP
        assert b"flame_agg_reduce_scaled" in err() and b"%d" % code in err()
        assert L.flame_agg_reduce_mixed(code, N.FLAME_F32, 0, fake, 1, 1, fake, 3, fake, None, None) == N.FLAME_ENOTSUP
        assert L.flame_agg_reduce_mixed(N.FLAME_BF16, code, 0, fake, 1, 1, fake, 3, fake, None, None) == N.FLAME_ENOTSUP
        assert L.flame_agg_trimmed(code, 0, fake, 1, 1, fake, 3, 1, None) == N.FLAME_ENOTSUP
        assert L.flame_agg_select(code, 0, fake, 1, 1, fake, 3, 1, None) == N.FLAME_ENOTSUP
        assert L.flame_update_stats(code, fake, 1, 1, fake, 3, fake, fake, fake, 1 << 30, None) == N.FLAME_ENOTSUP
        assert L.flame_update_dist(code, fake, 1, 1, fake, 3, fake, fake, fake, 1 << 30, None) == N.FLAME_ENOTSUP
        assert L.flame_update_gram(code, fake, 1, 1, fake, 3, fake, fake, fake, 1 << 30, None) == N.FLAME_ENOTSUP
        assert L.flame_fedopt_reduce_adapt(code, N.FLAME_FEDADAM, 0, fake, 1, 1, fake, 3, fake,
                                           0.9, 0.1, 0.99, 0.01, 0.1, 1e-3, None) == N.FLAME_ENOTSUP
        assert L.flame_scale_add_chunk_elems(code) == 0


def _run_mx_driver(timeout=900):
    """`make -f mx_driver.mk run-mx_driver` in tests/abi_asan: that file includes the Makefile of the other
    drivers and adds this one, and the output directory is tests/asan_drivers.py's, so the pytest process
    still builds the host-sanitized library once."""
    if asan_drivers._OUT is None:
        asan_drivers._OUT = tempfile.mkdtemp(prefix="flame_abi_asan_")
        atexit.register(shutil.rmtree, asan_drivers._OUT, ignore_errors=True)
    return subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "abi_asan"), "-f", "mx_driver.mk",
                           f"OUT={asan_drivers._OUT}", "run-mx_driver"], capture_output=True, text=True, timeout=timeout)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_mx_abi_validation_under_asan_ubsan():
    r = _run_mx_driver()
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mx abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
