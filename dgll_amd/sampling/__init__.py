from .base_sampler import Base_sampler, sugbraph  # noqa: F401
from .dgllsampler import DGLLNeighborSampler  # noqa: F401
from .fast_sampler import FastNeighborSampler  # noqa: F401
from .layerwise import FastGCNSampler, FastGCNSamplerFlat, Ladies, LadiesFlatWrs, LadiesWrs, LayerwiseSampler  # noqa: F401
from .neighbor import NeighborSampler  # noqa: F401
from .community import CommunityBatchLoader  # noqa: F401
from .edge import EdgePredictionSampler, PairBatch  # noqa: F401
from .subgraph import SAINTSampler, ShaDowKHopSampler, SubgraphWorkspace, node_subgraph  # noqa: F401
