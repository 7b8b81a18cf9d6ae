"""flame_agg_reduce_lowrank on the host: the symbols resolve, it is no launch branch, every refusal names it before any HIP call."""
import ctypes

from flame_amd import _native as N


def test_symbols_and_refusals():
    L, FAKE = N.lib(), ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    assert all(hasattr(L, n) for n in N.EXPORTS if "lowrank" in n) and not any("lowrank" in n for n in N.launch_branch_counts())
    assert L.flame_lowrank_tile() > 0 and L.flame_lowrank_stage_rows() % 2 == 0
    args = {"ad": N.FLAME_F32, "fd": N.FLAME_BF16, "flags": 0, "segs": FAKE, "n_segs": 1, "n_tiles": 2, "rows": FAKE, "n_rows": 16}
    call, err = lambda **kw: L.flame_agg_reduce_lowrank(*{**args, **kw}.values(), None), L.flame_last_error      # noqa: E731
    EINVAL, ENOTSUP = N.FLAME_EINVAL, N.FLAME_ENOTSUP
    table = [("segs", None, EINVAL, b"segment"), ("n_segs", 0, EINVAL, b"segment"), ("n_segs", -1, EINVAL, b"segment"), ("rows", None, EINVAL, b"row table"),
             ("n_rows", -1, EINVAL, b"n_rows"), ("n_tiles", 0, EINVAL, b"n_tiles"), ("n_tiles", -3, EINVAL, b"n_tiles"), ("n_tiles", 2 ** 24, EINVAL, b"n_tiles"),
             ("flags", N.FLAME_AGG_INIT_FIRST, EINVAL, b"unknown flags"), ("flags", 1 << 20, EINVAL, b"unknown flags")]
    table += [("ad", dt, ENOTSUP, b"aggregate dtype %d" % dt) for dt in (N.FLAME_BF16, N.FLAME_F64, N.FLAME_I32, 13, -1)]
    table += [("fd", dt, ENOTSUP, b"factor dtype %d" % dt) for dt in (N.FLAME_F16, N.FLAME_F64, N.FLAME_I64, N.FLAME_FP8_E4M3, N.FLAME_FP4_E2M1, 13, -1)]
    for k, v, status, text in table:
        assert call(**{k: v}) == status and b"flame_agg_reduce_lowrank" in err() and text in err(), (k, v, err())
