"""Random-walk node embeddings -- DeepWalk, node2vec and struc2vec -- on the device: walks over the CSR (dgll_amd/csrc/walk.hip),
struc2vec's structural distances (dgll_amd/csrc/struc_dtw.hip) and skip-gram with negative sampling (dgll_amd/csrc/sgns.hip).

The reference's `Graph Embedding/src/ge` package walks with Python `random` over a networkx graph (one `LabelEncoder.transform`
per step) and, for every (centre, context) pair, pushes a one-hot vector of length N through two dense matmuls and an N-way
softmax, then takes an SGD step over both whole tables (deepWalk.py:41-52, node2vec.py:53-91).  Here a batch of walks is one
launch (a lane per walk, Philox4x32-10 keyed by the seed, counter = (walk index, step, attempt)) and one training step over the
batch is three launches (scores, W_out update, W_in update).

Functions:
    random_walks(g, starts, length, p=1.0, q=1.0, seed=0, first_walk_index=0, stream=None, info=None, weighted=False, alias=None)
                                                         -> int32 [n, length], -1 after a dead end
    AliasTable.from_graph(g)                             per-row alias tables of the edge values, 8 bytes per edge, cached on g
    StrucContext.from_graph(g, opt1_reduce_len=True, opt2_reduce_sim_calc=True, opt3_num_layers=None)
                                                         struc2vec's multilayer context graph: degree sequences (BFS by SpMM),
                                                         pairs, DTW distances, stacked CSR + alias table + up-move thresholds
    struc_walks(ctx, starts, length, stay_prob, seed, first_walk_index, info=None, return_layers=False)
                                                         -> int32 [n, length] (and the layer of every entry)
    degree_sequences / select_pairs / struc_dtw          the three stages of the context graph on their own
    NoiseTable(weights) / NoiseTable.from_graph(g)       fixed-point cumulative noise distribution (in-degree^0.75 by default)
    sgns_negatives(walks, window, negatives, noise, seed, first_walk_index=0) -> int32 [n, L, 2W, K], -1 where there is no pair
    sgns_step(W_in, W_out, walks, window, negatives, noise, lr, seed, first_walk_index=0) -> loss sum (fp64 device scalar)
Classes (constructor arguments as in the reference, plus keyword-only extras, `weighted=False` among them):
    SkipGramModel(totalNodes, embedDim)                                                      skipgram.py:3-26
    DeepWalk(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr)             deepWalk.py:13-85
    Node2vec(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, p, q)       node2vec.py:13-118
    Struc2Vec(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, verbose, stay_prob, opt1_reduce_len,
              opt2_reduce_sim_calc, opt3_num_layers)                                         struc2vec.py:22-364
`graph` is a networkx graph (imported lazily; labels are encoded by their sorted order, as LabelEncoder does), a CSRGraph or a
DGraph.  The zero-means-default rules and their warnings are the reference's (randomWalkEmbedding.py:13-41, node2vec.py:23-32).

Documented differences (the reference's behaviour is not reproduced here):
  (a) Negative sampling replaces the N-way softmax: the loss is sum_pairs [-log sigma(u_c.v_t) - sum_k log sigma(-u_c.v_nk)] with K
      negatives per pair drawn from in-degree^0.75.  The softmax costs O(N D) per pair, and its gradient touches every row of W2.
  (b) A batch of walks is ONE synchronous step: every gradient is taken at the weights as the step found them and the updates are
      summed (not averaged: the reference steps once per pair with `lr`).  The reference steps after every pair.
  (c) The window is symmetric and excludes the centre: positions j-w .. j+w without j.  The reference's
      `range(max(0, j-w), min(j+w, len))` pairs a node with itself and drops j+w.
  (d) `numbOfWalksPerVertex == 0` selects the default (3).  The reference tests `== 3` (randomWalkEmbedding.py:25).
  (e) The draws are not bit-equal to Python's `random` or `np.random.choice` (a different generator); the node2vec transition
      probabilities are the reference's (tests/golden/node2vec_probs.npz).
  (f) Edge weights are ignored unless `weighted=True` is given (the default may change later).  With it every transition is
      multiplied by the edge's weight -- P(x | t, v) proportional to w_vx * bias(t, x), the reference's computeProbabilities
      (tests/golden/node2vec_probs_weighted.npz) -- drawn from a per-row alias table with the p/q rejection step on top.  An edge
      of weight 0 is never walked; a node whose out-weights sum to 0 ends the walk (the reference divides by 0 there).
      `DeepWalk(..., weighted=True)` is a weighted first-order walk, which the reference's DeepWalk does not have.
  (g) With `weighted=True` the first step is weighted too, as in standard node2vec; the reference's first step is uniform
      (node2vec.py:59).
  (h) struc2vec's distances are the exact DTW.  The reference calls fastdtw(radius=1), an approximation of it.
  (i) struc2vec's edge weights are exp(-(d - the smallest d of the row)) instead of exp(-d): the normalised weights -- the
      transition probabilities, gamma and the layer averages -- are the same, and a row of large distances does not underflow to
      all zeros (the reference divides by 0 there).  The walk draws from their float32 casts.
  (j) struc2vec pickles nothing: the context graph is built in the constructor and lives on the device; `temp_path` and `reuse`
      are accepted and ignored.  The reference's gensim `train` / `get_embeddings` are not provided; training is sgns_step.
DeepWalk on a node without out-edges ends the walk (the reference raises); node2vec stops there in both.
The classifiers and the plotting helpers are not provided.
"""
from .walks import AliasTable, random_walks, walk_info, MAX_ATTEMPTS  # noqa: F401
from .sgns import NoiseTable, sgns_negatives, sgns_step  # noqa: F401
from .struc2vec import DegreeSequences, StrucContext, degree_sequences, select_pairs, struc_dtw, struc_walks, up_thresholds  # noqa: F401
from .models import SkipGramModel, RandomWalkEmbedding, DeepWalk, Node2vec, Struc2Vec  # noqa: F401
