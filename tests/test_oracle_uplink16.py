"""Pin tests/golden/uplink16.npz (the REAL reference over bf16 / f16 updates into an fp32 model)
against the CPU oracle, as tests/test_oracle_golden.py pins the other fixtures, and against the
torch-CPU restatement the GPU tests use.  This pins the fixture, not the kernel."""
import os

import pytest
import torch

import scenarios as S
import uplink16_case as U
from oracle import oracle as O
from test_oracle_golden import make_oracle


def test_fixture_is_small_and_complete(golden):
    fx = golden("uplink16.npz")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uplink16.npz")
    assert os.path.getsize(path) <= 512 * 1024
    base, c0 = fx.weights("fedavg/base"), fx.weights("fedavg/client0")
    assert fx.meta["fedavg"]["n"] == 9 and all(t.dtype == torch.float32 for t in base.values())
    assert sorted((k, v.numel(), v.dtype) for k, v in c0.items()) == sorted(
        [(f"bf{n}", n, torch.bfloat16) for n in (77, 2048, 4099)] + [(f"h{n}", n, torch.float16) for n in (77, 2048, 4099)])
    assert [fx.meta[s]["rounds"] for s in U.SORTS] == [3, 3, 3]


@pytest.mark.parametrize("prefix", ["fedavg", "model"])
def test_oracle_fedavg_bitwise(golden, prefix):
    fx = golden("uplink16.npz")
    for label, got, exp in U.run_fedavg(fx, prefix, make_oracle, "cpu"):
        S.assert_bitwise(label, got, exp)


@pytest.mark.parametrize("prefix", ["fedavg", "model"])
def test_restatement_is_the_reference(golden, prefix):
    fx = golden("uplink16.npz")
    m = fx.meta[prefix]
    by_id = {e: (fx.weights(f"{prefix}/client{i}"), c) for i, (e, c) in enumerate(zip(m["end_ids"], m["counts"]))}
    base, exp = fx.weights(f"{prefix}/base"), fx.weights(f"{prefix}/out")
    got = {k: U.restate(base[k], [by_id[e][0][k] for e in m["order"]], [by_id[e][1] / m["total"] for e in m["order"]])
           for k in base}
    S.assert_bitwise(prefix, got, exp)


@pytest.mark.parametrize("sort", U.SORTS)
def test_oracle_fedopt(golden, sort):
    fx = golden("uplink16.npz")

    def state_is_fp32(r, opt):
        if opt.m_t is not None:
            assert all(t.dtype == torch.float32 for t in list(opt.m_t.values()) + list(opt.v_t.values()))
    U.check_fedopt(sort, U.run_fedopt(fx, sort, lambda s, **kw: O.OracleFedOPT(s, **kw), "cpu", each_round=state_is_fp32))
