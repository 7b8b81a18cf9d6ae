"""flame_mx_quantize on the host: the symbols resolve, the launch-branch table and the ABI version are unchanged,
and every refusal comes with its code and a message naming the entry point before any HIP call.  No GPU call."""
import ctypes
import itertools

WHO = b"flame_mx_quantize"


def test_refuses_without_gpu():
    from flame_amd import _native as N
    L = N.lib()
    assert {"flame_mx_quantize", "flame_mx_quantize_chunk_elems"} <= set(N.EXPORTS)
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert not any("quantize" in n for n in N.launch_branch_counts())
    assert L.flame_mx_quantize_chunk_elems() == 8192        # four passes of 256 lanes x 8 elements: 256 whole blocks
    assert [L.flame_chunk_elems(c) for c in (10, 11, 12)] == [4096, 4096, 8192]     # the reductions keep theirs
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host
    err = L.flame_last_error
    srcs = (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16)
    fmts = (N.FLAME_FP8_E4M3, N.FLAME_FP8_E5M2, N.FLAME_FP4_E2M1)
    codes = (*range(14), 21, -1)
    for sd, fd in itertools.product(codes, codes):
        if sd in srcs and fd in fmts:
            continue
        assert L.flame_mx_quantize(sd, fd, 0, fake, 1, 1, None) == N.FLAME_ENOTSUP, (sd, fd)
        assert WHO in err() and (b"f32, bf16 or f16" if sd not in srcs else b"e4m3, fp8 e5m2 or fp4 e2m1") in err(), err()
    for sd, fd in itertools.product(srcs, fmts):
        def call(flags=0, segs=fake, n_segs=1, n_chunks=1):
            return L.flame_mx_quantize(sd, fd, flags, segs, n_segs, n_chunks, None)
        for kw, word in (({"segs": None}, b"segment"), ({"n_segs": 0}, b"segment"), ({"n_segs": -2}, b"segment"),
                         ({"n_chunks": 0}, b"n_chunks"), ({"n_chunks": -4}, b"n_chunks"), ({"n_chunks": 2 ** 31}, b"n_chunks"),
                         ({"flags": 1}, b"unknown flags"), ({"flags": N.FLAME_AGG_XCD_MAP}, b"unknown flags"),
                         ({"flags": 1 << 20}, b"unknown flags")):
            assert call(**kw) == N.FLAME_EINVAL and WHO in err() and word in err(), (kw, err())
