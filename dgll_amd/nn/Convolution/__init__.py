"""Working replacement for the reference's broken package file (dgll/nn/Convolution/__init__.py:1-7 uses
absolute imports that fail); exports the same names plus the GAT/SAGE classes the modules define."""
from .gcnconv import gcnConv, GCN
from .gcn import GraphConvolution
from .sageconv import NeighborAggregator, sageConv, GraphSage
from .gatconv import gatConv, sparseGatConv, SpecialSpmm, SpecialSpmmFunction, GAT, SpGAT
from .ginconv import GinConv, GIN
from .gatv2conv import GATv2Conv, GATv2
from .dotgatconv import DotGatConv
from .transformerconv import TransformerConv, GraphTransformer
from .relgraphconv import RelGraphConv, RGCN
from .agnnconv import AGNNConv, AGNN
from .pnaconv import PNAConv, PNA
from .gineconv import GINEConv, GINE
from .cfconv import CFConv, ShiftedSoftplus
from .gatedgcnconv import GatedGCNConv, GatedGCN
from .resgatedconv import ResGatedGraphConv, ResGatedGCN
from .gmmconv import GMMConv, MoNet, degree_pseudo
from .genconv import GENConv, DeeperGCN
from .edgeconv import EdgeConv, DGCNN
from ...knn import KNNGraph, SegmentedKNNGraph

__all__ = ["gcnConv", "sageConv", "gatConv", "sparseGatConv", "GinConv", "GCN", "GIN",
           "GraphConvolution", "NeighborAggregator", "GraphSage", "SpecialSpmm", "SpecialSpmmFunction", "GAT", "SpGAT",
           "GATv2Conv", "GATv2", "DotGatConv", "TransformerConv", "GraphTransformer", "RelGraphConv", "RGCN", "AGNNConv", "AGNN",
           "PNAConv", "PNA", "GINEConv", "GINE", "CFConv", "ShiftedSoftplus", "GatedGCNConv", "GatedGCN",
           "ResGatedGraphConv", "ResGatedGCN", "GMMConv", "MoNet", "degree_pseudo", "GENConv", "DeeperGCN",
           "EdgeConv", "DGCNN", "KNNGraph", "SegmentedKNNGraph"]
