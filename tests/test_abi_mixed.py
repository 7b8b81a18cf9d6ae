"""flame_agg_reduce_mixed on the host: the symbol resolves, the header and the export list agree,
the launch-branch table and the ABI version are unchanged, every refusal comes with its code and a
message naming the entry point before any HIP call.  Then the same validation under ASan + UBSan
from a stand-alone C driver (tests/abi_asan/mixed_driver.c).  No GPU call, and no sanitizer inside Python."""
import ctypes
import itertools
import os
import re
import shutil

import pytest

import asan_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"flame_agg_reduce_mixed"


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbol_resolves_and_table_unchanged():
    N, L = _lib()
    assert "flame_agg_reduce_mixed" in N.EXPORTS and hasattr(L, "flame_agg_reduce_mixed")
    hdr = open(os.path.join(ROOT, "include", "flame_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(flame_[a-z0-9_]+)\s*\(", bare))) == sorted(N.EXPORTS)
    assert "int flame_agg_reduce_mixed(int client_dtype, int agg_dtype, unsigned flags," in hdr
    assert L.flame_agg_reduce_mixed.restype is ctypes.c_int and len(L.flame_agg_reduce_mixed.argtypes) == 11
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert not any("mixed" in n for n in N.launch_branch_counts())
    # the chunk is the client dtype's: one 4,096-byte slab tile
    assert L.flame_chunk_elems(N.FLAME_BF16) == L.flame_chunk_elems(N.FLAME_F16) == 2048 == N.FLAME_TILE_BYTES // 2
    # the header states the per-element contract and the refusals
    for text in ("round_C(f32(v_i[e]) * rate_i)", "round_f32(acc + f32(t))", "FLAME_AGG_INIT_FIRST is FLAME_ENOTSUP",
                 "FLAME_AGG_SEG_RATES is", "fedavg.py:93-104"):
        assert text in hdr, text


def test_mixed_refuses_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    B, H, F = N.FLAME_BF16, N.FLAME_F16, N.FLAME_F32

    def call(cd=B, ad=F, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=3, rates=fake, scales=None):
        return L.flame_agg_reduce_mixed(cd, ad, flags, segs, n_segs, n_chunks, clients, n_clients, rates, scales, None)
    err = L.flame_last_error
    # every pair but (bf16 | f16, f32): FLAME_ENOTSUP naming both dtypes
    codes = (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64, N.FLAME_I64, N.FLAME_I32, 6, 21, -1)
    for cd, ad in itertools.product(codes, codes):
        if cd in (B, H) and ad == F:
            continue
        assert call(cd=cd, ad=ad) == N.FLAME_ENOTSUP, (cd, ad)
        assert WHO in err() and b"client dtype %d" % cd in err() and b"aggregate dtype %d" % ad in err(), err()
    for cd in (B, H):
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
            assert call(cd=cd, scales=sc, n_clients=0) == N.FLAME_EINVAL and WHO in err() and b"n_clients" in err()
            assert call(cd=cd, scales=sc, n_clients=-3) == N.FLAME_EINVAL and b"n_clients" in err()
            assert call(cd=cd, scales=sc, rates=None) == N.FLAME_EINVAL and WHO in err() and b"rate array" in err()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="hipcc / make not available")
def test_mixed_abi_validation_under_asan_ubsan():
    r = asan_drivers.run_driver("mixed_driver")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mixed abi asan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
