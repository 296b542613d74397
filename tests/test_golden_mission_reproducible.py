"""Build container only (needs /root/reference; skipped where the reference does not exist): tests/golden/make_golden_mission.py is re-run into a
scratch directory and must reproduce the committed mission fixtures BYTE FOR BYTE -- they are outputs of the reference's own class."""
import filecmp
import os
import subprocess
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/src/dart_planner"), reason="the reference is only present in the build container")


def test_generator_reproduces_committed_fixtures(tmp_path):
    env = dict(os.environ, SE3MPC_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_mission.py")], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    for f in ("mission_cases.npz", "mission_cases.json"):
        assert filecmp.cmp(os.path.join(GOLDEN, f), os.path.join(str(tmp_path), f), shallow=False), f"{f} differs from what the generator writes"
    assert os.path.getsize(os.path.join(GOLDEN, "mission_cases.npz")) <= 1 << 20
