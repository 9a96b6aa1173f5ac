from .ComplEx import ComplEx
from .DistMult import DistMult
from .Model import Model
from .RESCAL import RESCAL
from .RotatE import RotatE
from .TransD import TransD
from .TransE import TransE
from .TransH import TransH
from .TransR import TransR

__all__ = ["Model", "TransE", "TransH", "TransD", "TransR", "DistMult", "ComplEx", "RotatE", "RESCAL"]
