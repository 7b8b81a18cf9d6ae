"""bench.py's plain / --full split and --dump-outputs, the CPU-checkable parts: a plain run asks
for no CPU baseline, the dump's sample is fixed by its seed and spans the tensor, and the files
are float32 / float64 within the size cap."""
import argparse
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_asks_for_no_cpu_baseline(monkeypatch):
    plain = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (plain.full, plain.cpu_clients, plain.steps, plain.warmup, plain.dump_outputs) == (False, 0, 7, 2, None)
    full = _parse(monkeypatch, "--full")
    assert full.full and full.cpu_clients == 128
    assert _parse(monkeypatch, "--full", "--cpu-clients", "16").cpu_clients == 16
    assert _parse(monkeypatch, "--dump-outputs", "d").dump_outputs == "d"


def test_dump_sample_is_fixed_sorted_distinct_and_spans_the_tensor():
    for numel, keep in ((25_000_000, 1 << 16), (1000, 999), (7, 3), (1 << 33, 1 << 10)):
        a = bench.dump_sample_indices(numel, keep)
        assert a.dtype == np.int64 and len(a) == keep
        assert np.array_equal(a, bench.dump_sample_indices(numel, keep))
        assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < numel
        # one pick per stratum
        edges = np.arange(keep + 1, dtype=np.int64) * numel // keep
        assert np.all(a >= edges[:-1]) and np.all(a < edges[1:])
    assert np.array_equal(bench.dump_sample_indices(5, 8), np.arange(5))
    assert not np.array_equal(bench.dump_sample_indices(10_000, 100), bench.dump_sample_indices(10_000, 100, seed=1))


def test_dump_outputs_writes_float_arrays_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    g = torch.Generator().manual_seed(3)
    outs = {"small": torch.randn(100, generator=g).to(torch.bfloat16).reshape(10, 10),
            "big": torch.randn(5000, generator=g),
            "wide": torch.randn(3000, generator=g, dtype=torch.float64)}
    args = argparse.Namespace(dump_outputs=str(tmp_path / "out"))
    bench.dump_outputs(args, 1, outs)
    assert not os.path.exists(args.dump_outputs)          # rank 0 writes
    bench.dump_outputs(args, 0, outs)
    got = {f[:-4]: np.load(os.path.join(args.dump_outputs, f)) for f in sorted(os.listdir(args.dump_outputs))}
    assert sorted(got) == ["big", "small", "wide"]
    assert sum(a.nbytes for a in got.values()) <= 4096
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], outs["small"].float().numpy().ravel())
    share = 4096 // 3
    assert got["big"].dtype == np.float32
    assert np.array_equal(got["big"], outs["big"].numpy()[bench.dump_sample_indices(5000, share // 4)])
    assert got["wide"].dtype == np.float64
    assert np.array_equal(got["wide"], outs["wide"].numpy()[bench.dump_sample_indices(3000, share // 8)])
    assert bench.dump_outputs(argparse.Namespace(dump_outputs=None), 0, outs) is None
