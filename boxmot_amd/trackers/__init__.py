from .boosttrack import BoostTrack
from .botsort import BotSort
from .bytetrack import ByteTrack
from .deepocsort import DeepOcSort, DeepOcSortPerClass
from .hybridsort import HybridSort, HybridSortPerClass
from .ocsort import OcSort
from .strongsort import StrongSort

__all__ = ["ByteTrack", "BotSort", "OcSort", "BoostTrack", "StrongSort", "DeepOcSort",
           "HybridSort", "DeepOcSortPerClass", "HybridSortPerClass"]
