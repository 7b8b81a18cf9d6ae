"""flame_sparse_index / flame_agg_reduce_sparse on the host: the symbols resolve, the launch-branch table is unchanged,
and every refusal names its entry point before any HIP call.  No GPU call."""
import ctypes

from flame_amd import _native as N

def test_symbols_sizes_and_refusals():
    L, FAKE = N.lib(), ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    assert all(hasattr(L, n) for n in N.EXPORTS if "sparse" in n) and sum("sparse" in n for n in N.EXPORTS) == 4
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1 and not any("sparse" in n for n in N.launch_branch_counts())
    assert L.flame_sparse_chunk_elems() == 4096 and [L.flame_sparse_index_scratch_bytes(*a) for a in ((6, 3), (0, 3), (6, 0), (2 ** 31, 3))] == [576, 0, 0, 0]
    need, err = L.flame_sparse_index_scratch_bytes(2, 3), L.flame_last_error
    index = {"segs": FAKE, "n_segs": 1, "n_chunks": 2, "indices": FAKE, "nnz": FAKE, "n_clients": 3, "bad": FAKE, "scratch": FAKE, "bytes": need}
    reduce = {"ad": N.FLAME_F32, "flags": 0, "segs": FAKE, "n_segs": 1, "n_chunks": 2, "indices": FAKE, "values": FAKE, "nnz": FAKE,
              "n_clients": 3, "rates": FAKE, "scales": None, "scratch": FAKE, "bytes": need}
    for fn, args, who in ((L.flame_sparse_index, index, b"flame_sparse_index"), (L.flame_agg_reduce_sparse, reduce, b"flame_agg_reduce_sparse")):
        call = lambda **kw: fn(*{**args, **kw}.values(), None)      # noqa: E731
        bad = [("segs", None, b"segment"), ("n_segs", 0, b"segment"), ("n_chunks", 0, b"n_chunks"), ("n_chunks", 2 ** 31, b"n_chunks"),
               ("n_clients", 0, b"n_clients"), ("indices", None, b"index pointer"), ("nnz", None, b"nnz"), ("scratch", None, b"scratch"),
               ("bytes", need - 1, b"%d needed" % need), ("bad", None, b"output array"), ("values", None, b"value pointer"),
               ("rates", None, b"rate array"), ("flags", N.FLAME_AGG_XCD_MAP, b"unknown flags"), ("flags", 1 << 20, b"unknown flags")]
        for k, v, text in bad:
            if k in args:
                assert call(**{k: v}) == N.FLAME_EINVAL and who in err() and text in err(), (k, err())
    for ad in (N.FLAME_BF16, N.FLAME_F64, N.FLAME_I32, N.FLAME_FP4_E2M1, 13, -1):
        assert call(ad=ad) == N.FLAME_ENOTSUP and b"flame_agg_reduce_sparse" in err() and b"aggregate dtype %d" % ad in err()
    for flag, text in ((N.FLAME_AGG_INIT_FIRST, b"INIT_FIRST"), (N.FLAME_AGG_SEG_RATES, b"SEG_RATES")):
        assert call(flags=flag) == call(flags=flag, scales=FAKE) == N.FLAME_ENOTSUP and text in err()
