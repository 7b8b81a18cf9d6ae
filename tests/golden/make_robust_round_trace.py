"""Generate ``robust_round_trace.json``: the trace of every (class, mode) pair of
``tests/test_robust_round_trace.py``, recorded from flame_amd/optimizer as of commit

    05583c5     (Add Multi-Krum aggregation on a pairwise fp64 Gram kernel)

the last one in which the plain, guarded, trimmed and krum rounds each popped, measured and decided
in a helper of their own.  The fixture pins what the optimizers decide and in which order they call
the engine; it is regenerated only when that is meant to change.  To check it, check that commit
out, copy this script and the test module in, run

    python tests/golden/make_robust_round_trace.py

(no GPU and no native library are needed) and diff the result against the committed file: the diff
is empty.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # repo root

import test_robust_round_trace as T  # noqa: E402


def main():
    traces = {}
    for sort in T.CLASSES:
        for mode in T.MODES:
            with pytest.MonkeyPatch.context() as mp:
                traces[f"{sort}-{mode}"] = T.run_case(sort, mode, mp)
    path = os.path.join(HERE, "robust_round_trace.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(t)}" for n, t in traces.items()) + "\n}\n")
    print(f"wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes, {len(traces)} cases)")


if __name__ == "__main__":
    main()
