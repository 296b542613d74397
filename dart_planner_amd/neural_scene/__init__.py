"""The mission layer's scene bookkeeping on the device: the reference's UncertaintyField.  PlaceholderNeuralScene and the
GlobalMissionPlanner's phase machine are not part of this package."""
from .uncertainty_field import UncertaintyField, UncertaintyRegion

__all__ = ["UncertaintyField", "UncertaintyRegion"]
