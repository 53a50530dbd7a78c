from .dit import DiT
from .mmdit import MMDiT
from .unett import UNetT

__all__ = ["DiT", "MMDiT", "UNetT"]
