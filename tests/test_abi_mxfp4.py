"""flame_agg_reduce_mxfp4 on the host: the symbol resolves, the header and the export list agree, the
launch-branch table and the ABI version are unchanged, every refusal comes with its code and a message
naming the entry point before any HIP call, and flame_agg_reduce_mx and every older reduce entry point
refuse the new element code.  Then the same validation under ASan + UBSan from a stand-alone C driver
(tests/abi_asan/mxfp4_driver.c, built by tests/abi_asan/mxfp4_driver.mk).  No GPU call, and no sanitizer
inside Python."""
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
WHO = b"flame_agg_reduce_mxfp4"


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbol_resolves_and_table_unchanged():
    N, L = _lib()
    assert "flame_agg_reduce_mxfp4" in N.EXPORTS and hasattr(L, "flame_agg_reduce_mxfp4")
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(flame_[a-z0-9_]+)\s*\(", bare))) == sorted(N.EXPORTS)
    assert "int flame_agg_reduce_mxfp4(int client_dtype, int agg_dtype, unsigned flags," in hdr
    vp = ctypes.c_void_p
    assert L.flame_agg_reduce_mxfp4.restype is ctypes.c_int
    assert L.flame_agg_reduce_mxfp4.argtypes == L.flame_agg_reduce_mx.argtypes == [
        ctypes.c_int, ctypes.c_int, ctypes.c_uint, vp, ctypes.c_int32, ctypes.c_int64, vp, vp, ctypes.c_int32, vp, vp, vp]
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert not any("mxfp4" in n for n in N.launch_branch_counts())
    # the code is the next free one, and the header's
    assert N.FLAME_FP4_E2M1 == 12 == N.FLAME_FP8_E5M2 + 1
    assert re.search(r"#define FLAME_FP4_E2M1 12\b", hdr)
    # the chunk: 32 elements per lane, one 4,096-byte tile of packed client bytes; the other codes keep theirs
    assert L.flame_chunk_elems(12) == 8192 == 2 * N.FLAME_TILE_BYTES
    assert L.flame_chunk_elems(N.FLAME_FP8_E4M3) == L.flame_chunk_elems(N.FLAME_FP8_E5M2) == 4096
    assert L.flame_chunk_elems(13) == 0 and L.flame_scale_add_chunk_elems(12) == 0
    # the header states the packing, the per-element contract, the equivalence and the refusals
    for text in ("flat element 2i is the LOW nibble of byte i", "HIGH nibble", "ceil(numel / 2) bytes",
                 "0, 0.5, 1, 1.5, 2, 3, 4, 6", "code 8 is -0", "the last high nibble is padding",
                 "b   = q_i[e >> 1];  c = (e & 1) ? b >> 4 : b & 15", "f32_e2m1(c) * f32_e8m0(s_i[e / 32])",
                 "one IEEE fp32 multiply", "denormals kept", "scale byte 255 gives NaN", "round_f32(x * scale_i)",
                 "round_f32(x * rate_i)", "round_f32(acc + t)", "bit for bit what", "dequantized update",
                 "client_tile_stride must be 0", "(e2m1, f32) is FLAME_ENOTSUP", "FLAME_AGG_SEG_RATES is FLAME_ENOTSUP",
                 "ANY alignment", "flame_chunk_elems(FLAME_FP4_E2M1) = 8,192"):
        assert text in hdr, text


def test_mxfp4_refuses_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    E2, F = N.FLAME_FP4_E2M1, N.FLAME_F32

    def call(cd=E2, ad=F, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, bscales=fake, n_clients=3, rates=fake,
             scales=None):
        return L.flame_agg_reduce_mxfp4(cd, ad, flags, segs, n_segs, n_chunks, clients, bscales, n_clients, rates, scales, None)
    err = L.flame_last_error
    # every pair but (e2m1, f32): FLAME_ENOTSUP naming both dtypes
    codes = (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64, N.FLAME_I64, N.FLAME_I32, N.FLAME_U8, N.FLAME_I8,
             N.FLAME_I16, N.FLAME_BOOL, N.FLAME_FP8_E4M3, N.FLAME_FP8_E5M2, E2, 13, 21, -1)
    for cd, ad in itertools.product(codes, codes):
        if (cd, ad) == (E2, F):
            continue
        assert call(cd=cd, ad=ad) == N.FLAME_ENOTSUP, (cd, ad)
        assert WHO in err() and b"client dtype %d" % cd in err() and b"aggregate dtype %d" % ad in err(), err()
    for sc in (None, fake):
        assert call(scales=sc, flags=N.FLAME_AGG_INIT_FIRST) == N.FLAME_ENOTSUP
        assert WHO in err() and b"INIT_FIRST" in err()
        assert call(scales=sc, flags=N.FLAME_AGG_INIT_FIRST | N.FLAME_AGG_XCD_MAP) == N.FLAME_ENOTSUP
        assert call(scales=sc, flags=N.FLAME_AGG_SEG_RATES) == N.FLAME_ENOTSUP
        assert WHO in err() and b"SEG_RATES" in err()
        assert call(scales=sc, flags=8) == N.FLAME_EINVAL and WHO in err() and b"unknown flags" in err()
        assert call(scales=sc, flags=1 << 20) == N.FLAME_EINVAL and b"unknown flags" in err()
        assert call(scales=sc, segs=None) == N.FLAME_EINVAL and WHO in err() and b"segment" in err()
        assert call(scales=sc, n_segs=0) == N.FLAME_EINVAL and WHO in err() and b"segment" in err()
        assert call(scales=sc, n_chunks=0) == N.FLAME_EINVAL and WHO in err() and b"n_chunks" in err()
        assert call(scales=sc, n_chunks=-4) == N.FLAME_EINVAL and b"n_chunks" in err()
        assert call(scales=sc, n_chunks=2 ** 31) == N.FLAME_EINVAL and b"n_chunks" in err()
        assert call(scales=sc, clients=None) == N.FLAME_EINVAL and WHO in err() and b"client pointer" in err()
        assert call(scales=sc, bscales=None) == N.FLAME_EINVAL and WHO in err() and b"block scale pointer" in err()
        assert call(scales=sc, n_clients=0) == N.FLAME_EINVAL and WHO in err() and b"n_clients" in err()
        assert call(scales=sc, n_clients=-3) == N.FLAME_EINVAL and b"n_clients" in err()
        assert call(scales=sc, rates=None) == N.FLAME_EINVAL and WHO in err() and b"rate array" in err()


def test_the_other_entry_points_refuse_the_new_code():
    """As they refuse any unknown code: FLAME_ENOTSUP before a launch (the tables are fake addresses)."""
    N, L = _lib()
    fake = ctypes.c_void_p(4096)
    err = L.flame_last_error
    code = N.FLAME_FP4_E2M1
    assert L.flame_agg_reduce_mx(code, N.FLAME_F32, 0, fake, 1, 1, fake, fake, 3, fake, None, None) == N.FLAME_ENOTSUP
    assert b"flame_agg_reduce_mx:" in err() and b"client dtype 12" in err()
    assert L.flame_agg_reduce_mx(N.FLAME_FP8_E4M3, code, 0, fake, 1, 1, fake, fake, 3, fake, None, None) == N.FLAME_ENOTSUP
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


def _run_mxfp4_driver(timeout=900):
    """`make -f mxfp4_driver.mk run-mxfp4_driver` in tests/abi_asan: that file includes the Makefile of the
    other drivers and adds this one, and the output directory is tests/asan_drivers.py's, so the pytest
    process still builds the host-sanitized library once."""
    if asan_drivers._OUT is None:
        asan_drivers._OUT = tempfile.mkdtemp(prefix="flame_abi_asan_")
        atexit.register(shutil.rmtree, asan_drivers._OUT, ignore_errors=True)
    return subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "abi_asan"), "-f", "mxfp4_driver.mk",
                           f"OUT={asan_drivers._OUT}", "run-mxfp4_driver"], capture_output=True, text=True, timeout=timeout)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_mxfp4_abi_validation_under_asan_ubsan():
    r = _run_mxfp4_driver()
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mxfp4 abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
