"""Drop-in `dgll` namespace: the reference's import paths (`from dgll import backend as F`,
`dgll.nn.Convolution.gcnconv`, `dgll.data.dgraph`, `dgll.sampling.dgllsampler`, `dgll.sampling.neighbor`, `dgll.sampling.edge`, `dgll.sampling.subgraph`, `dgll.dataloader`, `dgll.embedding`, `dgll.community`) resolved onto
the MI355X-native implementation in dgll_amd.  /root/reference/dgll/__init__.py:1 is `import torch as backend`;
here `backend` is dgll_amd.backend (torch + the missing aliases + HIP aggregation)."""
import importlib
import sys

import dgll_amd
from dgll_amd import backend  # noqa: F401

_ALIASES = {
    "dgll.backend": "dgll_amd.backend",
    "dgll.nn": "dgll_amd.nn",
    "dgll.nn.Convolution": "dgll_amd.nn.Convolution",
    "dgll.nn.Convolution.gcnconv": "dgll_amd.nn.Convolution.gcnconv",
    "dgll.nn.Convolution.gcn": "dgll_amd.nn.Convolution.gcn",
    "dgll.nn.Convolution.sageconv": "dgll_amd.nn.Convolution.sageconv",
    "dgll.nn.Convolution.gatconv": "dgll_amd.nn.Convolution.gatconv",
    "dgll.nn.Convolution.ginconv": "dgll_amd.nn.Convolution.ginconv",
    "dgll.nn.Convolution.gatv2conv": "dgll_amd.nn.Convolution.gatv2conv",
    "dgll.nn.Convolution.dotgatconv": "dgll_amd.nn.Convolution.dotgatconv",
    "dgll.nn.Convolution.transformerconv": "dgll_amd.nn.Convolution.transformerconv",
    "dgll.nn.Convolution.relgraphconv": "dgll_amd.nn.Convolution.relgraphconv",
    "dgll.nn.Convolution.agnnconv": "dgll_amd.nn.Convolution.agnnconv",
    "dgll.nn.Convolution.pnaconv": "dgll_amd.nn.Convolution.pnaconv",
    "dgll.nn.Convolution.gineconv": "dgll_amd.nn.Convolution.gineconv",
    "dgll.nn.Convolution.cfconv": "dgll_amd.nn.Convolution.cfconv",
    "dgll.nn.Convolution.gatedgcnconv": "dgll_amd.nn.Convolution.gatedgcnconv",
    "dgll.nn.Convolution.resgatedconv": "dgll_amd.nn.Convolution.resgatedconv",
    "dgll.nn.Convolution.gmmconv": "dgll_amd.nn.Convolution.gmmconv",
    "dgll.nn.Convolution.genconv": "dgll_amd.nn.Convolution.genconv",
    "dgll.nn.Convolution.edgeconv": "dgll_amd.nn.Convolution.edgeconv",
    "dgll.knn": "dgll_amd.knn",
    "dgll.nn.GlobalPooling": "dgll_amd.nn.GlobalPooling",
    "dgll.nn.GlobalPooling.Pooling": "dgll_amd.nn.GlobalPooling.Pooling",
    "dgll.data": "dgll_amd.data",
    "dgll.data.dgraph": "dgll_amd.data.dgraph",
    "dgll.sampling": "dgll_amd.sampling",
    "dgll.sampling.base_sampler": "dgll_amd.sampling.base_sampler",
    "dgll.sampling.dgllsampler": "dgll_amd.sampling.dgllsampler",
    "dgll.sampling.layerwise": "dgll_amd.sampling.layerwise",
    "dgll.sampling.neighbor": "dgll_amd.sampling.neighbor",
    "dgll.sampling.edge": "dgll_amd.sampling.edge",
    "dgll.sampling.community": "dgll_amd.sampling.community",
    "dgll.sampling.subgraph": "dgll_amd.sampling.subgraph",
    "dgll.dataloader": "dgll_amd.dataloader",
    "dgll.embedding": "dgll_amd.embedding",
    "dgll.community": "dgll_amd.community",
}
for _alias, _target in _ALIASES.items():
    sys.modules[_alias] = importlib.import_module(_target)
nn = sys.modules["dgll.nn"]
community = sys.modules["dgll.community"]
knn = sys.modules["dgll.knn"]
embedding = sys.modules["dgll.embedding"]      # `import dgll.embedding` finds the alias in sys.modules and binds no attribute itself
__version__ = dgll_amd.__version__
