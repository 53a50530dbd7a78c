from .backbones.dit import DiT
from .backbones.mmdit import MMDiT
from .backbones.unett import UNetT
from .cfm import CFM

__all__ = ["CFM", "DiT", "MMDiT", "UNetT"]
