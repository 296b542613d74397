"""Import-name shim: `dart_planner.neural_scene.uncertainty_field` -> `dart_planner_amd.neural_scene.uncertainty_field` (put
dart_planner_amd/compat on PYTHONPATH to run code written against the reference's package name)."""
from dart_planner_amd.neural_scene.uncertainty_field import *  # noqa: F401,F403
from dart_planner_amd.neural_scene.uncertainty_field import __dict__ as _d
globals().update({k: v for k, v in _d.items() if not k.startswith("__")})
