from .ComplEx import ComplEx
from .DistMult import DistMult
from .Model import Model
from .RotatE import RotatE
from .TransD import TransD
from .TransE import TransE
from .TransH import TransH

__all__ = ["Model", "TransE", "TransH", "TransD", "DistMult", "ComplEx", "RotatE"]
