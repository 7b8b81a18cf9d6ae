"""Generate ``engine_launch_trace.json``: the host-side launch trace of every case of
``tests/test_engine_launch_trace.py``.  The fixture pins what the launchers hand to the native
library; an entry is written once, from the engine as it stood BEFORE the change the entry guards,
and regenerated only when what reaches the library is meant to change.  The script only ever adds
the cases the fixture lacks; the entries it holds stay as they are.

Every case but the three families below was recorded from flame_amd/engine.py as of commit

    640eeb6e179ac0254cd67ace8ae8d11e19ebf83f

(the last one with a plan / stage / launch sequence written out per launch site).  To check those,
check that commit out, copy this script and the test module in, delete the fixture, run

    python tests/golden/make_engine_launch_trace.py

(the native library must be built; no GPU is needed) and compare the cases that commit can run.

The ``update_stats*``, ``update_gram*`` and ``trimmed_mean*`` cases were recorded from commit

    05583c5     (Add Multi-Krum aggregation on a pairwise fp64 Gram kernel)

the last one in which each of the three functions carried its own copy of the device
normalisation, the row building and the plan / scratch / launch / copy-back sequence.  There two
inline checks stop a trace over CPU tensors, so in a scratch checkout of that commit, and only
there, exactly these two lines were changed in each of ``update_stats``, ``update_gram`` and
``trimmed_mean``:

    if device.type != "cuda":        ->  never true (the RuntimeError is not raised for the tracer)
    if device.index is None:         ->  if device.type == "cuda" and device.index is None:

Since then the three functions take their device from ``engine._hip_device``, which the tracer
replaces.  ``engine.reduce_``, which ``trimmed_mean`` reaches through ``accumulate`` for integer
keys, has a device check of its own that neither edit covers: the tracer records that nested call
by label instead (see the test module's docstring).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root

import test_engine_launch_trace as T  # noqa: E402


def main():
    path = os.path.join(HERE, "engine_launch_trace.json")
    traces = {}
    if os.path.exists(path):
        with open(path) as f:
            traces = json.load(f)
    new = [name for name in sorted(T.CASES) if name not in traces]
    for name in new:
        traces[name] = T.run_case(name)
    with open(path, "w") as f:                                 # the held entries first, in their order
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(t)}" for n, t in traces.items()) + "\n}\n")
    print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes, {len(traces)} cases, {len(new)} new)")


if __name__ == "__main__":
    main()
