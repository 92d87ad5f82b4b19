"""tostore_amd -- MI355X-native exhaustive kNN behind ToStore's vectorSearch().

Only what the hot path needs: the HIP kernels + C-ABI (csrc/, built into
libtostore_hip.so), the ctypes binding (_ffi), and the host-side mirror of the
reference interface around the seam (backend, vector_index_manager, sharded).
"""
from . import _ffi  # noqa: F401
from .backend import (ATTR_NULL, HipAttr, HipGroups, HipMask, HipTags, HipVectorBackend, HipVectorIndex, NghSearchResult,  # noqa: F401
                      WhereIn, WhereRange, f64_order_key)
from .vector_index_manager import (VectorIndexManager, VectorSearchResult,  # noqa: F401
                                   distance_to_score, normalize_float32, to_float32)

__all__ = [
    "ATTR_NULL", "HipAttr", "HipGroups", "HipMask", "HipTags", "HipVectorBackend", "HipVectorIndex", "NghSearchResult", "VectorIndexManager",
    "VectorSearchResult", "WhereIn", "WhereRange", "distance_to_score", "f64_order_key", "normalize_float32", "to_float32",
]
