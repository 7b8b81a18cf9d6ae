"""Every refusal of the seven table entry points that stand outside the launch-branch table
(flame_agg_reduce_scaled, flame_agg_reduce_mixed, flame_agg_trimmed, flame_agg_select,
flame_update_stats / flame_update_dist, flame_update_gram, flame_noise_fill): the return code and
the whole message, one fault at a time, then two faults at once to fix which one is reported.
Host only: the pointers are fake and never dereferenced, every call fails before the first HIP call."""
import ctypes

import pytest


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


FAKE = ctypes.c_void_p(4096)
EINVAL, ENOTSUP = 1, 3
F32, BF16, F16, F64, I64, I32 = range(6)
INIT_FIRST, SEG_RATES, XCD_MAP = 1, 2, 4


def _check(call, cases):
    _, L = _lib()
    for kw, code, msg in cases:
        assert call(L, **kw) == code, (kw, L.flame_last_error())
        assert L.flame_last_error() == msg, (kw, L.flame_last_error())


def scaled(L, dtype=F32, flags=0, segs=FAKE, n_segs=1, n_chunks=1, clients=FAKE, n_clients=3, r32=FAKE, r64=FAKE,
           s32=FAKE, s64=FAKE):
    return L.flame_agg_reduce_scaled(dtype, flags, segs, n_segs, n_chunks, clients, n_clients, r32, r64, s32, s64, None)


SCALED = [
    (dict(segs=None), EINVAL, b"segment table is NULL or n_segs <= 0"),
    (dict(n_segs=0), EINVAL, b"segment table is NULL or n_segs <= 0"),
    (dict(n_segs=-2), EINVAL, b"segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0), EINVAL, b"n_chunks out of range: 0"),
    (dict(n_chunks=-4), EINVAL, b"n_chunks out of range: -4"),
    (dict(n_chunks=2 ** 31), EINVAL, b"n_chunks out of range: 2147483648"),
    (dict(n_clients=-1), EINVAL, b"n_clients < 0"),
    (dict(clients=None), EINVAL, b"client pointer table is NULL"),
    (dict(flags=SEG_RATES), ENOTSUP, b"flame_agg_reduce_scaled: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=INIT_FIRST, n_clients=0), EINVAL, b"FLAME_AGG_INIT_FIRST needs at least one client"),
    (dict(flags=8), EINVAL, b"flame_agg_reduce_scaled: unknown flags 0x8"),
    (dict(flags=1 << 20 | XCD_MAP), EINVAL, b"flame_agg_reduce_scaled: unknown flags 0x100004"),
    (dict(dtype=I64), ENOTSUP, b"flame_agg_reduce_scaled: integer dtype 4 not supported (float dtypes only)"),
    (dict(dtype=I32), ENOTSUP, b"flame_agg_reduce_scaled: integer dtype 5 not supported (float dtypes only)"),
    (dict(r32=None), EINVAL, b"flame_agg_reduce_scaled: rate array is NULL"),
    (dict(dtype=F64, r64=None), EINVAL, b"flame_agg_reduce_scaled: rate array is NULL"),
    (dict(s32=None), EINVAL, b"flame_agg_reduce_scaled: scale array is NULL"),
    (dict(dtype=F64, s64=None), EINVAL, b"flame_agg_reduce_scaled: scale array is NULL"),
    (dict(dtype=6), ENOTSUP, b"flame_agg_reduce_scaled: unknown dtype 6"),
    (dict(dtype=-1), ENOTSUP, b"flame_agg_reduce_scaled: unknown dtype -1"),
    # two faults: the earlier check speaks
    (dict(segs=None, n_chunks=0), EINVAL, b"segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0, clients=None), EINVAL, b"n_chunks out of range: 0"),
    (dict(clients=None, flags=SEG_RATES), EINVAL, b"client pointer table is NULL"),
    (dict(flags=SEG_RATES | 8), ENOTSUP, b"flame_agg_reduce_scaled: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8, dtype=I64), EINVAL, b"flame_agg_reduce_scaled: unknown flags 0x8"),
    (dict(dtype=I32, r32=None), ENOTSUP, b"flame_agg_reduce_scaled: integer dtype 5 not supported (float dtypes only)"),
    (dict(dtype=7, r32=None), EINVAL, b"flame_agg_reduce_scaled: rate array is NULL"),
    (dict(dtype=7, s32=None), EINVAL, b"flame_agg_reduce_scaled: scale array is NULL"),
    (dict(r32=None, s32=None), EINVAL, b"flame_agg_reduce_scaled: rate array is NULL"),
]


def mixed(L, cd=BF16, ad=F32, flags=0, segs=FAKE, n_segs=1, n_chunks=1, clients=FAKE, n_clients=3, rates=FAKE, scales=None):
    return L.flame_agg_reduce_mixed(cd, ad, flags, segs, n_segs, n_chunks, clients, n_clients, rates, scales, None)


MIXED = [
    (dict(cd=F32), ENOTSUP,
     b"flame_agg_reduce_mixed: client dtype 0 into aggregate dtype 0 is not supported (bf16 or f16 into f32 only)"),
    (dict(cd=F16, ad=F64), ENOTSUP,
     b"flame_agg_reduce_mixed: client dtype 2 into aggregate dtype 3 is not supported (bf16 or f16 into f32 only)"),
    (dict(segs=None), EINVAL, b"flame_agg_reduce_mixed: segment table is NULL or n_segs <= 0"),
    (dict(n_segs=0), EINVAL, b"flame_agg_reduce_mixed: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0), EINVAL, b"flame_agg_reduce_mixed: n_chunks out of range: 0"),
    (dict(n_chunks=2 ** 31), EINVAL, b"flame_agg_reduce_mixed: n_chunks out of range: 2147483648"),
    (dict(n_clients=0), EINVAL, b"flame_agg_reduce_mixed: n_clients < 1"),
    (dict(n_clients=-3), EINVAL, b"flame_agg_reduce_mixed: n_clients < 1"),
    (dict(clients=None), EINVAL, b"flame_agg_reduce_mixed: client pointer table is NULL"),
    (dict(rates=None), EINVAL, b"flame_agg_reduce_mixed: rate array is NULL"),
    (dict(flags=INIT_FIRST), ENOTSUP,
     b"flame_agg_reduce_mixed: FLAME_AGG_INIT_FIRST is not supported (a None-start aggregate takes the update's dtype)"),
    (dict(flags=SEG_RATES), ENOTSUP, b"flame_agg_reduce_mixed: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8), EINVAL, b"flame_agg_reduce_mixed: unknown flags 0x8"),
    (dict(cd=F16, scales=FAKE, flags=1 << 20), EINVAL, b"flame_agg_reduce_mixed: unknown flags 0x100000"),
    # two faults
    (dict(cd=I32, segs=None), ENOTSUP,
     b"flame_agg_reduce_mixed: client dtype 5 into aggregate dtype 0 is not supported (bf16 or f16 into f32 only)"),
    (dict(segs=None, n_chunks=0), EINVAL, b"flame_agg_reduce_mixed: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=-1, n_clients=0), EINVAL, b"flame_agg_reduce_mixed: n_chunks out of range: -1"),
    (dict(n_clients=0, clients=None), EINVAL, b"flame_agg_reduce_mixed: n_clients < 1"),
    (dict(clients=None, rates=None), EINVAL, b"flame_agg_reduce_mixed: client pointer table is NULL"),
    (dict(rates=None, flags=SEG_RATES), EINVAL, b"flame_agg_reduce_mixed: rate array is NULL"),
    (dict(flags=INIT_FIRST | SEG_RATES), ENOTSUP,
     b"flame_agg_reduce_mixed: FLAME_AGG_INIT_FIRST is not supported (a None-start aggregate takes the update's dtype)"),
    (dict(flags=SEG_RATES | 8), ENOTSUP, b"flame_agg_reduce_mixed: FLAME_AGG_SEG_RATES is not supported"),
]


def trimmed(L, dtype=F32, flags=0, segs=FAKE, n_segs=1, n_chunks=1, clients=FAKE, n_clients=5, trim_k=1):
    return L.flame_agg_trimmed(dtype, flags, segs, n_segs, n_chunks, clients, n_clients, trim_k, None)


TRIMMED = [
    (dict(segs=None), EINVAL, b"flame_agg_trimmed: segment table is NULL or n_segs <= 0"),
    (dict(n_segs=0), EINVAL, b"flame_agg_trimmed: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0), EINVAL, b"n_chunks out of range: 0"),
    (dict(n_chunks=2 ** 31), EINVAL, b"n_chunks out of range: 2147483648"),
    (dict(clients=None), EINVAL, b"flame_agg_trimmed: client pointer table is NULL"),
    (dict(trim_k=-1), EINVAL, b"flame_agg_trimmed: trim_k -1 outside [0, 16] (flame_agg_trimmed_max_k)"),
    (dict(trim_k=17, n_clients=64), ENOTSUP, b"flame_agg_trimmed: trim_k 17 outside [0, 16] (flame_agg_trimmed_max_k)"),
    (dict(n_clients=2), EINVAL, b"flame_agg_trimmed: n_clients 2 must exceed 2 * trim_k = 2"),
    (dict(n_clients=0, trim_k=0), EINVAL, b"flame_agg_trimmed: n_clients 0 must exceed 2 * trim_k = 0"),
    (dict(flags=SEG_RATES), ENOTSUP, b"flame_agg_trimmed: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8), EINVAL, b"flame_agg_trimmed: unknown flags 0x8"),
    (dict(dtype=I64), ENOTSUP, b"flame_agg_trimmed: integer dtype 4 not supported (float dtypes only)"),
    (dict(dtype=I32), ENOTSUP, b"flame_agg_trimmed: integer dtype 5 not supported (float dtypes only)"),
    (dict(dtype=6), ENOTSUP, b"flame_agg_trimmed: unknown dtype 6"),
    (dict(dtype=-1), ENOTSUP, b"flame_agg_trimmed: unknown dtype -1"),
    # two faults
    (dict(segs=None, n_chunks=0), EINVAL, b"flame_agg_trimmed: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0, clients=None), EINVAL, b"n_chunks out of range: 0"),
    (dict(clients=None, trim_k=-1), EINVAL, b"flame_agg_trimmed: client pointer table is NULL"),
    (dict(trim_k=17, n_clients=2), ENOTSUP, b"flame_agg_trimmed: trim_k 17 outside [0, 16] (flame_agg_trimmed_max_k)"),
    (dict(n_clients=2, flags=SEG_RATES), EINVAL, b"flame_agg_trimmed: n_clients 2 must exceed 2 * trim_k = 2"),
    (dict(flags=SEG_RATES | 8), ENOTSUP, b"flame_agg_trimmed: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8, dtype=I64), EINVAL, b"flame_agg_trimmed: unknown flags 0x8"),
]


def select(L, dtype=F32, flags=0, segs=FAKE, n_segs=1, n_chunks=1, clients=FAKE, n_clients=5, trim_k=1):
    return L.flame_agg_select(dtype, flags, segs, n_segs, n_chunks, clients, n_clients, trim_k, None)


SELECT = [
    (dict(segs=None), EINVAL, b"flame_agg_select: segment table is NULL or n_segs <= 0"),
    (dict(n_segs=-1), EINVAL, b"flame_agg_select: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0), EINVAL, b"n_chunks out of range: 0"),
    (dict(n_chunks=2 ** 31), EINVAL, b"n_chunks out of range: 2147483648"),
    (dict(clients=None), EINVAL, b"flame_agg_select: client pointer table is NULL"),
    (dict(trim_k=-1), EINVAL, b"flame_agg_select: trim_k -1 is negative"),
    (dict(n_clients=65536), ENOTSUP, b"flame_agg_select: n_clients 65536 exceeds 65535 (flame_agg_select_max_clients)"),
    (dict(n_clients=2), EINVAL, b"flame_agg_select: n_clients 2 must exceed 2 * trim_k = 2"),
    (dict(n_clients=7, trim_k=2 ** 31 - 1), EINVAL, b"flame_agg_select: n_clients 7 must exceed 2 * trim_k = 4294967294"),
    (dict(flags=SEG_RATES), ENOTSUP, b"flame_agg_select: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8), EINVAL, b"flame_agg_select: unknown flags 0x8"),
    (dict(dtype=I64), ENOTSUP, b"flame_agg_select: integer dtype 4 not supported (float dtypes only)"),
    (dict(dtype=I32), ENOTSUP, b"flame_agg_select: integer dtype 5 not supported (float dtypes only)"),
    (dict(dtype=9), ENOTSUP, b"flame_agg_select: unknown dtype 9"),
    (dict(dtype=-1), ENOTSUP, b"flame_agg_select: unknown dtype -1"),
    # two faults
    (dict(segs=None, clients=None), EINVAL, b"flame_agg_select: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=-4, trim_k=-1), EINVAL, b"n_chunks out of range: -4"),
    (dict(clients=None, trim_k=-1), EINVAL, b"flame_agg_select: client pointer table is NULL"),
    (dict(trim_k=-1, n_clients=65536), EINVAL, b"flame_agg_select: trim_k -1 is negative"),
    (dict(n_clients=65536, trim_k=40000), ENOTSUP,
     b"flame_agg_select: n_clients 65536 exceeds 65535 (flame_agg_select_max_clients)"),
    (dict(n_clients=2, flags=SEG_RATES), EINVAL, b"flame_agg_select: n_clients 2 must exceed 2 * trim_k = 2"),
    (dict(flags=SEG_RATES | 8, dtype=I64), ENOTSUP, b"flame_agg_select: FLAME_AGG_SEG_RATES is not supported"),
    (dict(flags=8, dtype=6), EINVAL, b"flame_agg_select: unknown flags 0x8"),
]


def _stats_call(name):
    def call(L, dtype=F32, segs=FAKE, n_segs=1, n_chunks=1, clients=FAKE, n_clients=3, out=FAKE, nonfinite=FAKE,
             scratch=FAKE, scratch_bytes=1 << 20):
        return getattr(L, name)(dtype, segs, n_segs, n_chunks, clients, n_clients, out, nonfinite, scratch, scratch_bytes,
                                None)
    return call


def _stats_cases(who, need):
    """flame_update_stats / _dist (need = 24: one workgroup x 3 clients x 8 bytes) and flame_update_gram
    (need = 32768: one 64 x 64 fp64 partial) refuse alike, bar the Gram's client bound."""
    w = who.encode()
    return [
        (dict(segs=None), EINVAL, w + b": segment table is NULL or n_segs <= 0"),
        (dict(n_segs=0), EINVAL, w + b": segment table is NULL or n_segs <= 0"),
        (dict(n_chunks=0), EINVAL, b"n_chunks out of range: 0"),
        (dict(n_chunks=2 ** 31), EINVAL, b"n_chunks out of range: 2147483648"),
        (dict(n_clients=0), EINVAL, w + b": n_clients <= 0"),
        (dict(n_clients=-2), EINVAL, w + b": n_clients <= 0"),
        (dict(clients=None), EINVAL, w + b": client pointer table is NULL"),
        (dict(dtype=I64), ENOTSUP, w + b": integer dtype 4 not supported (float dtypes only)"),
        (dict(dtype=I32), ENOTSUP, w + b": integer dtype 5 not supported (float dtypes only)"),
        (dict(dtype=6), ENOTSUP, w + b": unknown dtype 6"),
        (dict(dtype=-1), ENOTSUP, w + b": unknown dtype -1"),
        (dict(out=None), EINVAL, w + b": output array is NULL"),
        (dict(nonfinite=None), EINVAL, w + b": output array is NULL"),
        (dict(scratch=None), EINVAL, w + b": scratch buffer is NULL or too small (1048576 bytes, %d needed)" % need),
        (dict(scratch_bytes=need - 1), EINVAL,
         w + b": scratch buffer is NULL or too small (%d bytes, %d needed)" % (need - 1, need)),
        (dict(scratch_bytes=-8), EINVAL, w + b": scratch buffer is NULL or too small (-8 bytes, %d needed)" % need),
        # two faults
        (dict(segs=None, n_chunks=0), EINVAL, w + b": segment table is NULL or n_segs <= 0"),
        (dict(n_chunks=0, n_clients=0), EINVAL, b"n_chunks out of range: 0"),
        (dict(n_clients=0, clients=None), EINVAL, w + b": n_clients <= 0"),
        (dict(clients=None, dtype=I64), EINVAL, w + b": client pointer table is NULL"),
        (dict(dtype=I32, out=None), ENOTSUP, w + b": integer dtype 5 not supported (float dtypes only)"),
        (dict(dtype=7, scratch=None), ENOTSUP, w + b": unknown dtype 7"),
        (dict(out=None, scratch=None), EINVAL, w + b": output array is NULL"),
    ]


GRAM_ONLY = [
    (dict(n_clients=1025), ENOTSUP, b"flame_update_gram: n_clients 1025 exceeds 1024 (flame_update_gram_max_clients)"),
    (dict(n_clients=1025, clients=None), ENOTSUP,
     b"flame_update_gram: n_clients 1025 exceeds 1024 (flame_update_gram_max_clients)"),
    (dict(n_chunks=0, n_clients=1025), EINVAL, b"n_chunks out of range: 0"),
]


def noise(L, dtype=F32, segs=FAKE, n_segs=1, n_chunks=1, streams=FAKE, starts=FAKE, std=1.0):
    return L.flame_noise_fill(dtype, segs, n_segs, n_chunks, streams, starts, 7, 1, std, None)


NOISE = [
    (dict(segs=None), EINVAL, b"flame_noise_fill: segment table is NULL or n_segs <= 0"),
    (dict(n_segs=0), EINVAL, b"flame_noise_fill: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0), EINVAL, b"flame_noise_fill: n_chunks out of range: 0"),
    (dict(n_chunks=2 ** 31), EINVAL, b"flame_noise_fill: n_chunks out of range: 2147483648"),
    (dict(dtype=I64), ENOTSUP,
     b"flame_noise_fill: float dtypes only (integer and bool tensors get no noise), got dtype 4"),
    (dict(dtype=I32), ENOTSUP,
     b"flame_noise_fill: float dtypes only (integer and bool tensors get no noise), got dtype 5"),
    (dict(dtype=9), ENOTSUP, b"flame_noise_fill: unknown dtype 9"),
    (dict(dtype=-1), ENOTSUP, b"flame_noise_fill: unknown dtype -1"),
    (dict(std=-1.0), EINVAL, b"flame_noise_fill: std must be a finite number >= 0, got -1"),
    (dict(std=float("nan")), EINVAL, b"flame_noise_fill: std must be a finite number >= 0, got nan"),
    (dict(std=float("inf")), EINVAL, b"flame_noise_fill: std must be a finite number >= 0, got inf"),
    (dict(std=1e39), EINVAL, b"flame_noise_fill: std 1e+39 rounds to an infinite fp32"),
    (dict(streams=None), EINVAL, b"flame_noise_fill: the streams / starts array is NULL"),
    (dict(starts=None), EINVAL, b"flame_noise_fill: the streams / starts array is NULL"),
    # two faults
    (dict(segs=None, n_chunks=0), EINVAL, b"flame_noise_fill: segment table is NULL or n_segs <= 0"),
    (dict(n_chunks=0, dtype=I64), EINVAL, b"flame_noise_fill: n_chunks out of range: 0"),
    (dict(dtype=I64, std=-1.0), ENOTSUP,
     b"flame_noise_fill: float dtypes only (integer and bool tensors get no noise), got dtype 4"),
    (dict(dtype=9, streams=None), ENOTSUP, b"flame_noise_fill: unknown dtype 9"),
    (dict(std=-1.0, streams=None), EINVAL, b"flame_noise_fill: std must be a finite number >= 0, got -1"),
    (dict(std=1e39, starts=None), EINVAL, b"flame_noise_fill: std 1e+39 rounds to an infinite fp32"),
]


@pytest.mark.parametrize("call,cases", [
    (scaled, SCALED), (mixed, MIXED), (trimmed, TRIMMED), (select, SELECT),
    (_stats_call("flame_update_stats"), _stats_cases("flame_update_stats", 24)),
    (_stats_call("flame_update_dist"), _stats_cases("flame_update_dist", 24)),
    (_stats_call("flame_update_gram"), _stats_cases("flame_update_gram", 32768) + GRAM_ONLY),
    (noise, NOISE),
], ids=["reduce_scaled", "reduce_mixed", "trimmed", "select", "update_stats", "update_dist", "update_gram", "noise_fill"])
def test_refusal_code_and_whole_message(call, cases):
    _check(call, cases)


def test_abi_unchanged():
    N, L = _lib()
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    assert [L.flame_chunk_elems(d) for d in (F32, BF16, F16, F64, I64, I32)] == [1024, 2048, 2048, 512, 512, 1024]
    assert (EINVAL, ENOTSUP) == (N.FLAME_EINVAL, N.FLAME_ENOTSUP)
    assert (INIT_FIRST, SEG_RATES, XCD_MAP) == (N.FLAME_AGG_INIT_FIRST, N.FLAME_AGG_SEG_RATES, N.FLAME_AGG_XCD_MAP)
    assert (F32, BF16, F16, F64, I64, I32) == (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64, N.FLAME_I64, N.FLAME_I32)
