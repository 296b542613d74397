"""Import-name shim: `dart_planner.planning.global_mission_planner` -> `dart_planner_amd.planning.global_mission_planner` (put
dart_planner_amd/compat on PYTHONPATH to run code written against the reference's package name)."""
from dart_planner_amd.planning.global_mission_planner import *  # noqa: F401,F403
from dart_planner_amd.planning.global_mission_planner import __dict__ as _d
globals().update({k: v for k, v in _d.items() if not k.startswith("__")})
