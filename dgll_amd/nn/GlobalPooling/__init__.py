"""Graph-level read-out (reference: dgll/nn/GlobalPooling/Pooling.py) and pooling by selection (select.py)."""
from .Pooling import Pooling, maxPooling, meanPooling, segments_of, sumPooling  # noqa: F401
from .select import SAGPooling, SortPooling, TopKPooling, global_sort_pool  # noqa: F401

__all__ = ["sumPooling", "meanPooling", "maxPooling", "Pooling", "TopKPooling", "SAGPooling", "SortPooling", "global_sort_pool"]
