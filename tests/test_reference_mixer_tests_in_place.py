"""Build container only (needs /root/reference; skipped on the GPU box): the reference's OWN motor-mixer and motor-model test files are run in
place, unchanged, twice -- against the reference itself (under the identity-units stand-in of tests/golden/make_golden.py) and against the
mirrors of dart_planner_amd/hardware over the product kernels compiled for the host (tests/emu, through ref_contract_plugin and
ref_mixer_plugin) -- and the two runs must pass, fail and error on the same tests.

The files: tests/test_motor_mixing.py, tests/hardware/test_motor_mixer_units.py, tests/hardware/test_motor_model.py,
tests/integration/test_hover_integration.py, tests/test_motor_mixing_safety.py.

Figures of this run: 40 passed, 16 failed, 13 errors out of 69 on both.  tests/hardware/test_motor_mixer_units.py wraps a MockMotorModel written in
that file, not a QuadraticMotorModel: the mirror keeps its own arithmetic on the device for such a model and calls the model's methods on the host
(dart_planner_amd/hardware/motor_mixer.py)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/tests"
FILES = ["test_motor_mixing.py", "hardware/test_motor_mixer_units.py", "hardware/test_motor_model.py", "integration/test_hover_integration.py",
         "test_motor_mixing_safety.py"]
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is only present in the build container")


def run_in_place(pythonpath, plugins):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath), PYTHONDONTWRITEBYTECODE="1", DART_ENV="test", DART_SECRET_KEY="golden", DART_ZMQ_SECRET="golden")
    with tempfile.TemporaryDirectory() as cwd:
        r = subprocess.run([sys.executable, "-m", "pytest", "-c", os.devnull, "--rootdir", REF, "--confcutdir", REF] + [x for p in plugins for x in ("-p", p)]
                           + ["-p", "no:cacheprovider", "-q", "-rA"] + [os.path.join(REF, f) for f in FILES], cwd=cwd, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
    sets = {k: set(re.findall(rf"^{k} (\S+?)(?: - .*)?$", r.stdout, re.M)) for k in ("PASSED", "FAILED", "ERROR")}
    return sets, r.stdout


def test_reference_mixer_test_files_pass_and_fail_alike_on_the_reference_and_on_the_mirror():
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
    mirror, out = run_in_place([os.path.join(ROOT, "dart_planner_amd", "compat"), ROOT, os.path.join(ROOT, "tests", "emu")], ["ref_contract_plugin", "ref_mixer_plugin"])
    print({k: len(v) for k, v in ref.items()}, {k: len(v) for k, v in mirror.items()})
    for k in ("PASSED", "FAILED", "ERROR"):
        assert mirror[k] == ref[k], (k, sorted(mirror[k] ^ ref[k]), out[-3000:])
    assert len(ref["PASSED"]) >= 40, ref_out[-3000:]
