"""flame_agg_reduce_sign on the host: the symbols resolve, the launch-branch table is unchanged, and every refusal names the
entry point before any HIP call.  No GPU call."""
import ctypes
import os

from flame_amd import _native as N

NAMES = ("flame_agg_reduce_sign", "flame_sign_chunk_elems")


def test_symbols_and_refusals():
    L, FAKE, err = N.lib(), ctypes.c_void_p(4096), N.lib().flame_last_error     # FAKE is never dereferenced: every call fails on the host
    header = open(os.path.join(os.path.dirname(N.PKG), "include", "flame_amd.h")).read()
    assert all(n in N.EXPORTS and hasattr(L, n) and f"{n}(" in header for n in NAMES) and sorted(n for n in N.EXPORTS if "sign" in n) == sorted(NAMES)
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1 and not any("sign" in n for n in N.launch_branch_counts())
    assert L.flame_sign_chunk_elems() == 16384
    args = {"ad": N.FLAME_F32, "flags": 0, "segs": FAKE, "n_segs": 1, "n_chunks": 2, "bits": FAKE, "scales": FAKE, "n_clients": 3, "rates": FAKE}
    call = lambda **kw: L.flame_agg_reduce_sign(*{**args, **kw}.values(), None)      # noqa: E731
    odd = ctypes.c_void_p(4100)
    for k, v, text in [("segs", None, b"segment"), ("n_segs", 0, b"segment"), ("n_chunks", 0, b"n_chunks"), ("n_chunks", 2 ** 31, b"n_chunks"),
                       ("n_clients", 0, b"n_clients"), ("bits", None, b"bit pointer"), ("scales", None, b"scale pointer"), ("rates", None, b"rate array"),
                       ("bits", odd, b"8-byte aligned"), ("scales", odd, b"8-byte aligned"), ("segs", odd, b"8-byte aligned"),
                       ("flags", N.FLAME_AGG_XCD_MAP, b"unknown flags"), ("flags", 1 << 20, b"unknown flags")]:
        assert call(**{k: v}) == N.FLAME_EINVAL and b"flame_agg_reduce_sign" in err() and text in err(), (k, err())
    for ad in (N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64, N.FLAME_I32, N.FLAME_FP4_E2M1, 13, -1):
        assert call(ad=ad) == N.FLAME_ENOTSUP and b"flame_agg_reduce_sign" in err() and b"aggregate dtype %d" % ad in err()
    for flag, text in ((N.FLAME_AGG_INIT_FIRST, b"INIT_FIRST"), (N.FLAME_AGG_SEG_RATES, b"SEG_RATES")):
        assert call(flags=flag) == N.FLAME_ENOTSUP and b"flame_agg_reduce_sign" in err() and text in err()
