"""pytest plugin (TEST INFRASTRUCTURE, build container only): lets the reference's own motor-mixer and motor-model test files run *in place,
unchanged* against this package on a box without a GPU by pointing the mirrors of dart_planner_amd/hardware at the host-emulated kernels.
Loaded next to ref_contract_plugin (which does the same for the planner, controller and simulator mirrors):

  PYTHONPATH=dart_planner_amd/compat:.:tests/emu python -m pytest -c /dev/null --rootdir=/tmp \
      -p ref_contract_plugin -p ref_mixer_plugin -p no:cacheprovider /root/reference/tests/test_motor_mixing.py

On a GPU box drop both plugins: the mirrors then use libse3mpc.so."""
import build_emu
from numpy_backend import TorchCpuBackend


def pytest_configure(config):
    from dart_planner_amd import capi
    from dart_planner_amd.ops import Ops
    from dart_planner_amd.hardware import motor_mixer, motor_model
    ops = Ops(TorchCpuBackend(), capi.Library(build_emu.build()))
    motor_mixer.MotorMixer._get_ops = lambda self: ops
    motor_model.QuadraticMotorModel._get_ops = lambda self: ops
