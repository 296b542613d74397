"""The mission layer's scene bookkeeping on the device: the reference's UncertaintyField.  PlaceholderNeuralScene is not part
of this package; the GlobalMissionPlanner's phase machine is dart_planner_amd.planning.global_mission_planner."""
from .uncertainty_field import UncertaintyField, UncertaintyRegion

__all__ = ["UncertaintyField", "UncertaintyRegion"]
