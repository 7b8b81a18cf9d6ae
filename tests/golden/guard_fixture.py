"""Reader and checker of ``fedavg_clipped.npz`` (made by make_golden_guard.py from the reference's
own clip + FedAvg), shared by the CPU and the GPU test."""
from __future__ import annotations

import collections

import torch

Case = collections.namedtuple("Case", "clip base updates counts ends ref_scale ref_norm out norm_tol")


def load(fx) -> Case:
    m = fx.meta
    pos = {e: i for i, e in enumerate(m["end_ids"])}
    idx = [pos[e] for e in m["order"]]                    # the reference cache's iterkeys() order
    return Case(clip=float(m["clip_threshold"]), base=fx.weights("base"),
                updates=[fx.weights(f"client{i}") for i in idx], counts=[m["counts"][i] for i in idx],
                ends=[m["end_ids"][i] for i in idx], ref_scale=[m["ref_scale"][i] for i in idx],
                ref_norm=[m["ref_total_norm"][i] for i in idx], out=fx.weights("out"),
                norm_tol=float(m["norm_tol"]))


def check(case: Case, records, got) -> None:
    """The same clients are clipped; scales agree within norm_tol; every f32 key is within
    2 * norm_tol + 2^-22 (rel-L2) of the reference's model.  (bf16 keys: the bitwise oracle tests.)"""
    assert len(records) == len(case.ref_scale)
    assert [r.scale != 1.0 for r in records] == [s != 1.0 for s in case.ref_scale]
    assert sum(r.scale != 1.0 for r in records) == 3
    for r, s, n in zip(records, case.ref_scale, case.ref_norm):
        print(f"scale {r.scale!r} vs reference {s!r}; norm {r.norm!r} vs reference {n!r} (norm_tol {case.norm_tol:.3e})")
        assert abs(r.scale - s) <= case.norm_tol * s, (r, s)
    bound = 2 * case.norm_tol + 2.0 ** -22
    checked = 0
    for k, e in case.out.items():
        if e.dtype != torch.float32:
            continue
        g = got[k].detach().cpu()
        assert g.dtype == e.dtype and g.shape == e.shape
        l2 = ((g.double() - e.double()).norm() / e.double().norm()).item()
        print(f"{k}: rel-L2 against the reference's model {l2:.3e} (bound {bound:.3e})")
        assert l2 <= bound, (k, l2, bound)
        checked += 1
    assert checked >= 1
