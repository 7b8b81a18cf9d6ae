"""Generate ``engine_launch_trace.json``: the host-side launch trace of every case of
``tests/test_engine_launch_trace.py``, recorded from flame_amd/engine.py as of commit

    640eeb6e179ac0254cd67ace8ae8d11e19ebf83f

(the last one with a plan / stage / launch sequence written out per launch site).  The fixture
pins what the launchers hand to the native library; it is regenerated only when that is meant to
change.  To check it, check that commit out, copy this script and the test module in, run

    python tests/golden/make_engine_launch_trace.py

(the native library must be built; no GPU is needed) and diff the result against the
committed file: the diff is empty.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root

import test_engine_launch_trace as T  # noqa: E402


def main():
    traces = {name: T.run_case(name) for name in sorted(T.CASES)}
    path = os.path.join(HERE, "engine_launch_trace.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(t)}" for n, t in traces.items()) + "\n}\n")
    print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes, {len(traces)} cases)")


if __name__ == "__main__":
    main()
