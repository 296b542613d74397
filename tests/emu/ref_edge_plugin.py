"""pytest plugin (TEST INFRASTRUCTURE, build container only): lets the reference's own latency-buffer test file run *in place, unchanged*
against this package on a box without a GPU by pointing the mirrors of dart_planner_amd/utils/latency_buffer.py and
dart_planner_amd/control/onboard_controller.py at the host-emulated kernels:

  PYTHONPATH=dart_planner_amd/compat:.:tests/emu python -m pytest -c /dev/null --rootdir=/tmp \
      -p ref_edge_plugin -p no:cacheprovider /root/reference/tests/utils/test_latency_buffer.py

On a GPU box drop the plugin: the mirrors then use libse3mpc.so."""
import build_emu
from numpy_backend import TorchCpuBackend


def pytest_configure(config):
    from dart_planner_amd import capi
    from dart_planner_amd.ops import Ops
    from dart_planner_amd.utils import latency_buffer
    from dart_planner_amd.control import onboard_controller
    ops = Ops(TorchCpuBackend(), capi.Library(build_emu.build()))
    latency_buffer.DroneStateLatencyBuffer._get_ops = lambda self: ops
    onboard_controller.OnboardController._get_ops = lambda self: ops
