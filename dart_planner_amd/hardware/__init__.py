"""The arithmetic between the controller's command and the actuators: the reference's motor model and MotorMixer on the device
(DESIGN.md 5.7d).  The transports of its hardware back ends (MAVLink, AirSim) are not part of this package."""
