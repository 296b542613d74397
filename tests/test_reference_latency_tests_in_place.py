"""Build container only (needs /root/reference; skipped on the GPU box): the reference's OWN latency-buffer test file,
tests/utils/test_latency_buffer.py, is run in place, unchanged, twice -- against the reference itself (under the identity-units stand-in of
tests/golden/make_golden.py) and against the mirrors of dart_planner_amd/utils/latency_buffer.py over the product kernels compiled for the host
(tests/emu, through ref_edge_plugin) -- and the two runs must pass and fail on the same tests.

Figures of this run: 14 passed, 2 failed out of 16 on both.  The two failures (TestDroneStateLatencyBuffer::test_drone_state_delay_compensation
and ::test_drone_state_continuous_operation) read ``.magnitude`` of the delayed state's position, which under identity units is a plain ndarray
on either side."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/tests"
FILES = ["utils/test_latency_buffer.py"]
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is only present in the build container")


def run_in_place(pythonpath, plugins):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath), PYTHONDONTWRITEBYTECODE="1", DART_ENV="test", DART_SECRET_KEY="golden", DART_ZMQ_SECRET="golden")
    with tempfile.TemporaryDirectory() as cwd:
        r = subprocess.run([sys.executable, "-m", "pytest", "-c", os.devnull, "--rootdir", REF, "--confcutdir", REF] + [x for p in plugins for x in ("-p", p)]
                           + ["-p", "no:cacheprovider", "-q", "-rA"] + [os.path.join(REF, f) for f in FILES], cwd=cwd, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
    sets = {k: set(re.findall(rf"^{k} (\S+?)(?: - .*)?$", r.stdout, re.M)) for k in ("PASSED", "FAILED", "ERROR")}
    return sets, r.stdout


def test_reference_latency_test_file_passes_and_fails_alike_on_the_reference_and_on_the_mirror():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden
    finally:
        sys.path.pop(0)
    with tempfile.TemporaryDirectory() as standins:
        os.makedirs(os.path.join(standins, "pint"))
        for name, text in (("__init__.py", make_golden.PINT_INIT), ("errors.py", make_golden.PINT_ERRORS)):
            with open(os.path.join(standins, "pint", name), "w") as f:
                f.write(text)
        ref, ref_out = run_in_place([standins, "/root/reference/src"], [])
    mirror, out = run_in_place([os.path.join(ROOT, "dart_planner_amd", "compat"), ROOT, os.path.join(ROOT, "tests", "emu")], ["ref_edge_plugin"])
    print({k: len(v) for k, v in ref.items()}, {k: len(v) for k, v in mirror.items()})
    for k in ("PASSED", "FAILED", "ERROR"):
        assert mirror[k] == ref[k], (k, sorted(mirror[k] ^ ref[k]), out[-3000:])
    assert len(ref["PASSED"]) == 14 and len(ref["FAILED"]) == 2 and not ref["ERROR"], ref_out[-3000:]
