"""Sessions stepped by the caller's own per-tile rates (reference package bitrate_selection/simulators/)."""
from ..utils.qoe import QoEModel  # noqa: F401
from .simulator import BatchedSimulator, Simulator, schedule_digits  # noqa: F401
