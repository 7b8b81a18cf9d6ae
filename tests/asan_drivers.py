"""Runs one of the stand-alone sanitizer drivers of tests/abi_asan (`make run-<driver>`).  Every
driver links the same host-sanitized library, so one pytest process shares one temporary output
directory: make builds the library for whichever test asks first and reuses it for the rest.  The
directory is removed when the process exits.  Nothing sanitized is loaded into Python."""
import atexit
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_OUT = None


def run_driver(name, timeout=900):
    """The CompletedProcess of `make run-<name>` (stdout / stderr captured as text)."""
    global _OUT
    if _OUT is None:
        _OUT = tempfile.mkdtemp(prefix="flame_abi_asan_")
        atexit.register(shutil.rmtree, _OUT, ignore_errors=True)
    return subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "abi_asan"), f"OUT={_OUT}", f"run-{name}"],
                          capture_output=True, text=True, timeout=timeout)
