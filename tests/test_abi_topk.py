"""flame_topk_select on the host: the symbols resolve, the launch-branch table and the ABI version are unchanged, and
every refusal carries its code and names the entry point before any HIP call.  No GPU call."""
import ctypes

from flame_amd import _native as N

WHO = b"flame_topk_select"


def test_symbols_sizes_and_refusals():
    L, FAKE, err = N.lib(), ctypes.c_void_p(4096), N.lib().flame_last_error     # FAKE is never dereferenced
    assert {"flame_topk_select", "flame_topk_chunk_elems", "flame_topk_scratch_bytes"} <= set(N.EXPORTS)
    assert all(hasattr(L, n) for n in N.EXPORTS if "topk" in n) and not any("sparse" in n for n in N.EXPORTS if "topk" in n)
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1 and not any("topk" in n for n in N.launch_branch_counts())
    assert L.flame_topk_chunk_elems() == 4096
    # per segment three histograms of 2,048 counters and 16 bytes of state, per chunk two counters
    assert [L.flame_topk_scratch_bytes(*a) for a in ((2, 5), (0, 5), (2, 0), (2, 2 ** 31))] == [2 * (3 * 2048 * 4 + 16) + 5 * 8, 0, 0, 0]
    need = L.flame_topk_scratch_bytes(1, 2)
    args = {"sd": N.FLAME_F32, "flags": 0, "segs": FAKE, "n_segs": 1, "n_chunks": 2, "k": FAKE, "scratch": FAKE, "bytes": need}
    call = lambda **kw: L.flame_topk_select(*{**args, **kw}.values(), None)      # noqa: E731
    for kw, text in (({"segs": None}, b"segment"), ({"n_segs": 0}, b"segment"), ({"n_chunks": 0}, b"n_chunks"),
                     ({"n_chunks": 2 ** 31}, b"n_chunks"), ({"flags": 2}, b"unknown flags"), ({"flags": 1 << 20}, b"unknown flags"),
                     ({"k": None}, b"k array"), ({"scratch": None}, b"scratch"), ({"bytes": need - 1}, b"%d needed" % need)):
        assert call(**kw) == N.FLAME_EINVAL and WHO in err() and text in err(), (kw, err())
    for sd in (N.FLAME_F64, N.FLAME_I64, N.FLAME_I32, N.FLAME_FP8_E4M3, 13, -1):
        assert call(sd=sd) == N.FLAME_ENOTSUP and WHO in err() and b"source dtype %d" % sd in err()
    for sd in (N.FLAME_BF16, N.FLAME_F16):              # a base goes with an fp32 source
        assert call(sd=sd, flags=N.FLAME_TOPK_BASE) == N.FLAME_ENOTSUP and WHO in err() and b"FLAME_TOPK_BASE" in err()
    # one segment of more than 2^19 chunks is a key of 2^31 elements or more
    big = 2 ** 19 + 1
    assert call(n_chunks=big, bytes=L.flame_topk_scratch_bytes(1, big)) == N.FLAME_ENOTSUP and WHO in err() and b"2^31" in err()
