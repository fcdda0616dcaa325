/*
 * dgll_hip.h -- C ABI of libdgll_hip.so, the MI355X (gfx950) sparse GNN aggregation engine that sits
 * behind the dgll.nn conv-layer API.
 *
 * This is the drop-in boundary of the hot path.  The reference's own native
 * boundary has the same shape -- two extern "C" launchers taking borrowed device pointers and plain
 * ints (/root/reference/dgll/FusedKernel/gcn_fused_kernel.cu:190-195 and :238-244, bound from Python by
 * gcn_extension.cpp:5-18,46-55).  Each entry point below cites the reference call site it serves.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller and borrowed for the duration of the launch
 *     (as gcn_extension.cpp:46-55 borrows tensor.data_ptr()); nothing is allocated or freed on the data
 *     path; scratch memory is passed in by the caller (`workspace`);
 *   - `stream` is a hipStream_t passed as void*; launches are ASYNCHRONOUS on it (the reference launcher
 *     synchronises the whole device, gcn_fused_kernel.cu:229 -- deliberately not reproduced);
 *   - return value: 0 on success, negative DGLL_ERR_* otherwise; dgll_hip_last_error() gives the text
 *     (the reference calls exit(1), gcn_fused_kernel.cu:224-227 -- deliberately not reproduced);
 *   - CSR: int64 rowptr[n_rows+1], int32 col[nnz], optional fp32 val[nnz] (NULL = all ones);
 *     dense matrices are row-major with an explicit leading dimension in ELEMENTS;
 *   - dtypes: DGLL_F32 or DGLL_BF16 storage, fp32 accumulation always;
 *   - re-entrant and thread-safe: no global mutable state besides the thread-local error string.
 */
#ifndef DGLL_HIP_H
#define DGLL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGLL_HIP_ABI_VERSION 2

enum { DGLL_OK = 0, DGLL_ERR_INVALID = -1, DGLL_ERR_HIP = -2, DGLL_ERR_UNSUPPORTED = -3, DGLL_ERR_WORKSPACE = -4 };
enum { DGLL_F32 = 0, DGLL_BF16 = 1 };
enum { DGLL_REDUCE_SUM = 0, DGLL_REDUCE_MEAN = 1 };
/* epilogue bit-mask applied to a finished output row: y = act(scale*acc + bias) */
enum { DGLL_EPI_NONE = 0, DGLL_EPI_BIAS = 1, DGLL_EPI_RELU = 2 };

typedef struct dgll_csr_plan dgll_csr_plan; /* opaque: load-balancing schedule of one CSR structure */

/* ---- library -------------------------------------------------------------------------------------- */
int dgll_hip_abi_version(void);
const char* dgll_hip_last_error(void);
/* Fills name (<= name_len bytes), compute-unit count and total global memory of `device`. */
int dgll_hip_device_info(int device, char* name, int name_len, int* compute_units, int64_t* global_mem_bytes);

/* Diagnostics only: kernel tuning knobs used by tools/spmm_tune.py (0 unroll depth, 1 rows per wavefront, 2 flags,
 * 3 default long-row threshold).  Not part of the data path; not thread-safe.
 * Key 16: cap on the grid of the resident-weights bf16 transform (gemm_bf16_res_kernel).  0 = no cap (shipped default);
 * v > 0: min(default grid, max(16, v / 16 * 16)) workgroups -- whole groups of 16, which the pairing of column-split partners
 * needs.  With 16 a persistent workgroup wraps to its second row block after 16 x 512 rows, so the kernel's steady state is
 * reachable at test sizes (tests/test_dense_steady_gpu.py); dgll_hip_debug_transform_choice reports the capped grid. */
int dgll_hip_debug_tune(int key, int value);

/* Diagnostics only, touches no device: the kernel a dgll_hip_spmm_csr* launch of this description gets under the current
 * knobs -- the launch path calls the same function.  kernel: 0 wave-per-row, 1 row-per-slot, 2 row-group, 3 flattened;
 * epv / lpr: elements per lane and lanes per row; spr: slots per row (0 for kernels 0 and 3); unroll / prefetch: gathers in
 * flight per lane and the next-row index prefetch; the grid is (row_blocks + chunk_blocks, grid_y).  nnz / n_chunks /
 * n_flat are the plan's (ignored when has_plan is 0; n_flat = 0: no flattened schedule).                           */
struct dgll_spmm_choice {
    int kernel, epv, lpr, spr, unroll, prefetch, rows_per_wave, grid_y;
    int64_t row_blocks, chunk_blocks;
};
int dgll_hip_debug_spmm_choice(int x_dtype, int y_dtype, int feat, int64_t n_rows, int has_plan, int64_t nnz,
                               int64_t n_chunks, int64_t n_flat, int weighted, int accumulate, int gate, int aligned16,
                               int only_long, struct dgll_spmm_choice* out);

/* Diagnostics only, touches no device: the kernel a launch of the fused GAT passes of this description gets under the current
 * knobs (key 9) -- the launch path calls the same function.  In: pass 0 forward / 1 rows of A / 2 rows of A^T; rowscore: attn2
 * INSTEAD of T; drop: dropout drawn in the kernel; phase: the rows pass's `accumulate` / `phase`; t_stride (0 = heads) and the
 * 16-byte alignment of the gathered-side score arrays (T; pass 2: S and dd of the columns); sd_out / score_epilogue: those
 * optional outputs are asked for; the in-row facts: the first score array starts right behind the first gathered row's last
 * column, t_stride floats are one row pitch, the second array (pass 2) sits one float after the first, pad_bytes of padding per
 * gathered row; nnz / n_chunks / n_long are the plan's (ignored when has_plan is 0); y_aligned: the output rows admit the
 * wavefront finalize kernel's four-column stores.
 * Out: generation 1 / 2; generation 2: gat2_kernel<.., lpr, nh, 4, kind, inrow, trow, drop>; generation 1: lph lanes per head,
 * `unroll` gathers in flight; the grid is (chunk_blocks + row_blocks, grid_y); finalize: 0 none, 1 a wavefront, 2 a workgroup
 * per long row.  A refusal returns its code (also in `error`) with `message` (static storage) as the error text.          */
struct dgll_gat_choice {
    int generation, kind, trow, drop, inrow, epv, lpr, nh, lph, unroll, grid_y, rows_per_wave, finalize, error;
    int64_t row_blocks, chunk_blocks;
    const char* message;
};
int dgll_hip_debug_gat_choice(int pass, int dtype, int heads, int fo, int mode, int edge_scale, int rowscore, int drop, int phase,
                              int t_stride, int t_aligned16, int dd_aligned16, int sd_out, int score_epilogue,
                              int score_behind_row, int score_pitch_equal, int second_follows, int64_t pad_bytes, int has_plan,
                              int64_t n_rows, int64_t nnz, int64_t n_chunks, int64_t n_long, int y_aligned,
                              struct dgll_gat_choice* out);

/* Diagnostics only, touches no device: the kernel a dgll_hip_transform_bf16* launch of this description gets under the current
 * knobs (keys 4, 11, 16) -- the launch path calls the same function.  In: N, K1, K2 (0 = no second operand pair); whether an
 * input ReLU mask, fp32 output, row scale, addend, bf16 out_gate, gate_bits is given; out_aligned: the output is 16-byte
 * aligned with ldo % 8 == 0; ldw_equal: ldw1 == ldw2; dual: dgll_hip_transform_bf16_dual (K2 and the epilogue inputs are
 * ignored); M rows; n_cu: the device's compute-unit count (the launch path passes the real one; <= 0 means 256).
 * Out: kernel 0 = the 4-wave gemm_bf16_nt_kernel<nt> (one 128-row block per workgroup; ntw .. per_cu are 0), 1 = the persistent
 * resident-weights gemm_bf16_res_kernel<ntw, .., nc, cs, colsplit, .., epi, .., dual>: rows_per_block rows per block, lds_bytes of
 * dynamic LDS, per_cu workgroups per CU, `workgroups` in the grid, which walk row_sequences (= workgroups / colsplit) interleaved
 * sequences of the n_blocks row blocks -- a workgroup runs more than one block when n_blocks > row_sequences;
 * bits_in_epilogue: sign bits asked for (bits_out) are written by the kernel's epilogue (1) or by sign_bits_kernel afterwards (0).
 * A refusal returns its code (also in `error`) with `message` (static storage) as the error text.                           */
struct dgll_transform_choice {
    int kernel, nt, ntw, nc, cs, colsplit, epi, dual, rows_per_block, lds_bytes, per_cu, bits_in_epilogue, error;
    int64_t workgroups, row_sequences, n_blocks;
    const char* message;
};
int dgll_hip_debug_transform_choice(int N, int K1, int K2, int mask, int out_f32, int row_scale, int addend, int out_gate,
                                    int gate_bits, int out_aligned, int ldw_equal, int dual, int64_t M, int n_cu,
                                    struct dgll_transform_choice* out);

/* ---- CSR schedule ----------------------------------------------------------------------------------
 * Built once per adjacency structure (the reference builds its adjacency once per graph,
 * nn/utils/utils.py:171,179).  Rows longer than `long_row_threshold` nonzeros (<= 0 selects the default,
 * 128) are split into chunks that are reduced in a fixed order, so results are bit-reproducible and
 * power-law rows do not serialise the launch.  Synchronises `stream` (it reads a count back).
 * long_row_threshold < 0 is the caller's guarantee that NO row exceeds the default threshold (a sampled block whose
 * fan-out is at most 128): the plan is then created on the host alone -- no scan, no allocation, no synchronisation --
 * which matters for blocks that are rebuilt every mini-batch.                                            */
int dgll_hip_csr_plan_create(void* stream, const int64_t* rowptr, int64_t n_rows, int64_t nnz,
                             int long_row_threshold, dgll_csr_plan** out_plan);
void dgll_hip_csr_plan_destroy(dgll_csr_plan* plan);
/* Scratch bytes dgll_hip_spmm_csr / dgll_hip_gat_* need for `feat` output columns with this plan. */
size_t dgll_hip_csr_plan_workspace_bytes(const dgll_csr_plan* plan, int feat);
int64_t dgll_hip_csr_plan_num_long_rows(const dgll_csr_plan* plan);
int64_t dgll_hip_csr_plan_num_chunks(const dgll_csr_plan* plan);

/* ---- a1 / a3 / a7-forward: Y[n_rows, feat] = epilogue( reduce_j A[i,j] * X[j, :] ) -------------------
 * Serves F.spmm(adj, support) (dgll/nn/Convolution/gcnconv.py:31, gcn.py:39), torch.sparse.mm
 * (Evaluation/PPI/gcn_model.py:76), the K-axis mean/sum of NeighborAggregator (sageconv.py:33-36, a
 * constant-degree CSR) and SpecialSpmmFunction.forward (gatconv.py:66-69).  With the transposed CSR it is
 * also every grad_X = A^T.g (autograd of the above; gatconv.py:80).
 * `plan` may be NULL (every row is then handled by one wavefront).  `val` may be NULL (unweighted).
 * `bias` is fp32[feat] and only read when epilogue has DGLL_EPI_BIAS.                                   */
int dgll_hip_spmm_csr(void* stream, const dgll_csr_plan* plan,
                      const int64_t* rowptr, const int32_t* col, const float* val,
                      const void* X, int64_t ldx, int x_dtype,
                      void* Y, int64_t ldy, int y_dtype,
                      int64_t n_rows, int64_t n_cols, int feat,
                      int reduce, int epilogue, const float* bias,
                      void* workspace, size_t workspace_bytes);

/* Same launch with two extras used by the partitioned (multi-GPU) path, where one destination row's neighbours are
 * split over an owned-columns CSR and a halo-columns CSR: `accumulate` != 0 adds the row already in Y before the
 * epilogue (Y = act(scale * (A.X + Y) + bias)); `row_scale` (fp32[n_rows], may be NULL) replaces the reduce's own
 * 1/nnz(row) so both halves share the full degree.  `accumulate` == 2 is the increment form, Y += gate(scale * A.X)
 * with rows that have no edge left untouched (no bias / ReLU): the halo half and the reduction of returned gradient
 * pieces touch a fraction of the rows, and re-writing all of them cost more than the gathers.                  */
int dgll_hip_spmm_csr_ex(void* stream, const dgll_csr_plan* plan,
                         const int64_t* rowptr, const int32_t* col, const float* val,
                         const void* X, int64_t ldx, int x_dtype, void* Y, int64_t ldy, int y_dtype,
                         int64_t n_rows, int64_t n_cols, int feat, int reduce, int epilogue, const float* bias,
                         void* workspace, size_t workspace_bytes, const float* row_scale, int accumulate);

/* dgll_hip_spmm_csr_ex plus a fused ReLU backward for the layer BELOW: where gate[i, c] <= 0 (gate: [n_rows, ldg] of Y's
 * dtype, the forward activations relu produced; may be NULL) the output element is written as 0.  Used when Y is the
 * gradient w.r.t. those activations (sageconv.py:81-82 applies the activation last): the separate masking pass over
 * [N, F] disappears.                                                                                              */
int dgll_hip_spmm_csr_gated(void* stream, const dgll_csr_plan* plan,
                            const int64_t* rowptr, const int32_t* col, const float* val,
                            const void* X, int64_t ldx, int x_dtype, void* Y, int64_t ldy, int y_dtype,
                            int64_t n_rows, int64_t n_cols, int feat, int reduce, int epilogue, const float* bias,
                            void* workspace, size_t workspace_bytes, const float* row_scale, int accumulate,
                            const void* gate, int64_t ldg);

/* ---- a7 backward: edge_out[k] = <G[row(k), :], B[col[k], :]> ------------------------------------------
 * The sampled dense-dense product SpecialSpmmFunction.backward computes through a dense N x N matmul
 * (gatconv.py:76-78).  G and B share `dtype`; both must be 16-byte aligned with leading dimensions padded to
 * a multiple of 16 bytes; feat <= 64 vectors of 16 bytes (256 fp32 / 512 bf16 columns).                      */
int dgll_hip_sddmm_csr(void* stream, const int64_t* rowptr, const int32_t* col,
                       const void* G, int64_t ldg, const void* B, int64_t ldb, int dtype,
                       float* edge_out, int64_t n_rows, int feat);

/* ---- a6 / a8 / a9: fused multi-head edge-softmax + aggregation: three gather passes behind one entry point (csrc/edge.hip) ------
 * All `heads` attention heads of one layer in one launch (the reference loops heads in Python, gatconv.py:168,196), nothing stored
 * per edge.  Over the rows i of a CSR matrix A [n_rows x n_cols], with per-node scores s_i = a_k[:fo].h_i^k, t_j = a_k[fo:].h_j^k
 * (gatconv.py:122-125 without materialising edge_h):
 *     mode 0 (sparseGatConv)  w_ij = exp(-leakyrelu_alpha(s_i + t_j))                                        (gatconv.py:125)
 *     mode 1 (gatConv on the adjacency's nonzeros)  softmax_j(+leakyrelu), the row maximum subtracted        (gatconv.py:34-36,53-54)
 *     out_i = act( sum_j w_ij scale_ij h_j / sum_j w_ij ),  act = ELU when apply_elu                         (gatconv.py:143-145)
 * scale_ij: `edge_scale` (fp32 [nnz, heads] or NULL), applied after the row sum exactly as gatconv.py:129-135 orders it.
 *   DGLL_GAT_FORWARD     rowptr / col / plan = A.  Reads h [n_cols, heads * fo], row_score = S fp32 [n_rows, heads] and the t_j
 *                        (below); writes out [n_rows, heads * fo], rowsum and (mode 1) rowmax, fp32 [n_rows, heads], kept for the
 *                        backward.  Mode 0 only: raw != 0 leaves the row un-normalised (numerator in out, denominator in rowsum);
 *                        accumulate != 0 adds the numerator / denominator already there, then (unless raw) normalises and applies
 *                        the ELU -- a row whose neighbours are split over an owned-columns and a halo-columns CSR.
 *   DGLL_GAT_ROWS        the same A.  Reads h, row_score = S, the t_j, out, grad_out, rowsum, (mode 1) rowmax; writes dn [n_rows,
 *                        heads * fo], grad_score = grad_S fp32 [n_rows, heads] and dd_i -- into dd (compact fp32 [n_rows, heads])
 *                        and / or, with sd, as {s_i[0:heads], dd_i[0:heads]} side by side every sd_stride (>= 2 heads) floats, which
 *                        the transposed pass gathers with ONE line fill: a separate buffer or a slot in the padding of the dn rows.
 *                        At least one of dd / sd.  `phase`:
 *                          DGLL_GAT_ROWS_STORED_FIRST    dd_i = -dn_i . hp_i, hp_i recovered from the stored output row; the first (or
 *                                                        only) launch over these rows;
 *                          DGLL_GAT_ROWS_STORED_FURTHER  a further launch over another column half (grad_S +=, dn / dd left alone);
 *                          DGLL_GAT_ROWS_EXACT_ONLY      DECLARED the only launch over these rows (mode 0): dd_i from the pass's own
 *                                                        dot products, sum_j w_ij (dn_i . h_j) / den_i -- exact in the stored operands;
 *                          DGLL_GAT_ROWS_EXACT_FIRST / _MIDDLE / _LAST   the exact dd_i over SEVERAL column halves (ds_i is bilinear in
 *                                                        the sums (sum c.dot, sum c, sum w.dot), so no launch can finalise its own
 *                                                        share): the first writes dn and parks the sums in partial3, the last adds
 *                                                        partial3 and writes dd and grad_S.  partial3: fp32 [n_rows, 3 * heads],
 *                                                        caller-owned, the same buffer for every phase; dd required.
 *   DGLL_GAT_TRANSPOSED  rowptr / col / plan = A^T (n_rows = the source nodes), perm[k] = A's edge slot of A^T's k-th edge (needed
 *                        with edge_scale only).  Reads dn (gathered), h (its own rows), row_score = T of its rows, col_score = S and
 *                        col_dd = dd of its columns (both every col_score_stride floats: col_score = sd, col_dd = sd + heads,
 *                        col_score_stride = sd_stride after a rows pass that wrote sd), (mode 1) rowmax of its columns; writes grad_h
 *                        [n_rows, heads * fo] and grad_score = grad_T fp32 [n_rows, heads].  attn1 / attn2 / grad_s_rows (all three
 *                        or none; attn* fp32 [heads * fo] laid out like a row of h, grad_s_rows = grad_S of this pass's rows): when
 *                        S = H.a1, T = H.a2 per head, their own share grad_S[j] * attn1 + grad_T[j] * attn2 of grad_h is added in the
 *                        epilogue instead of by a separate product and add.
 * The t_j of the forward and the rows pass (the passes are bound by cache-line fills per edge: four for a 512-byte row plus one for
 * every separate per-node array gathered per edge):
 *   col_score  read at col_score[j * col_score_stride + head] (0 = heads, else >= heads): a compact [n_cols, heads] array, or a slot
 *              in the PADDING of the h rows themselves (a 47-class bf16 row is 94 of 128 bytes: col_score = (float*)((char*)h + 96),
 *              col_score_stride = ld_h * elem_size / 4) -- the in-row form: the score shares the row's cache line and costs nothing;
 *   attn2      with a NULL col_score (mode 0, no edge_scale; rows pass: DGLL_GAT_ROWS_EXACT_ONLY): t_j = h_j . attn2 per head is FORMED
 *              from the gathered row, no score is fetched per edge (bf16: attn2 rounded to bf16 for the packed dot product, as the
 *              caller's score product rounds it).  The gathers use 32-bit byte offsets: h of at most 2^24 rows (n_cols) and 4 GB,
 *              DGLL_ERR_UNSUPPORTED past that -- fill col_score instead.
 * Attention dropout drawn in the kernels (gatconv.py:132: the row sum keeps every edge, the aggregation loses a fraction drop_p of
 * them, survivors scaled by 1 / (1 - drop_p)): drop_seed != NULL, mode 0 without edge_scale, one launch over the rows (no raw /
 * accumulate, DGLL_GAT_ROWS_EXACT_ONLY), col_score XOR attn2, 32-bit node ids.  drop_p in [0, 1), anything else is
 * DGLL_ERR_INVALID.  drop_seed is a DEVICE pointer to two 32-bit words, read by the kernels: a captured graph whose seed words are
 * rewritten between replays draws a fresh mask on every replay; the backward passes must be given the words the forward read.  The
 * multiplier of edge (row i, column j), head k is a pure function of (seed, i, j, k) that each pass evaluates for the edges it walks
 * (the transposed pass swaps the ids back; duplicate (i, j) entries share a draw).  There is no in-row form with dropout.
 * Matrices of `dtype`, pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned bases.  fo (per-head width) is a multiple of the
 * vector (4 fp32 / 8 bf16 columns); mode 1 and edge_scale need a power of two of them (the host pads each head with zero columns).
 * plan (NULL: every row is handled by one wavefront) splits long rows, whose partials need `workspace` of
 * dgll_hip_gat_workspace_bytes() bytes.  An empty pass (n_rows <= 0) is DGLL_OK.  Nothing is launched before every check has passed;
 * no pass allocates, synchronises or reads anything back: the calls can be captured into a graph.                                  */
enum { DGLL_GAT_FORWARD = 0, DGLL_GAT_ROWS = 1, DGLL_GAT_TRANSPOSED = 2 };
enum { DGLL_GAT_ROWS_STORED_FIRST = 0, DGLL_GAT_ROWS_STORED_FURTHER = 1, DGLL_GAT_ROWS_EXACT_ONLY = 3,
       DGLL_GAT_ROWS_EXACT_FIRST = 4, DGLL_GAT_ROWS_EXACT_MIDDLE = 5, DGLL_GAT_ROWS_EXACT_LAST = 6 };
typedef struct dgll_gat_desc {
    int pass; int dtype; int mode; int apply_elu;
    const dgll_csr_plan* plan; const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols;
    int heads; int fo; float alpha;
    void* workspace; size_t workspace_bytes;
    const float* edge_scale;
    double drop_p; const uint32_t* drop_seed;
    const void* h; int64_t ld_h;
    void* out; int64_t ld_out;
    const void* grad_out; int64_t ld_grad_out;
    void* dn; int64_t ld_dn;
    void* grad_h; int64_t ld_grad_h;
    const float* row_score;
    const float* col_score; int col_score_stride; const float* col_dd;
    const float* attn1; const float* attn2; const float* grad_s_rows;
    float* rowsum; float* rowmax;
    float* dd; float* sd; int sd_stride;
    float* grad_score;
    float* partial3;
    int raw; int accumulate; int phase;
} dgll_gat_desc;
int dgll_hip_gat_pass(void* stream, const dgll_gat_desc* d);
/* Scratch for the long-row partials of a pass over this plan's structure (0 without long rows or a plan). */
size_t dgll_hip_gat_workspace_bytes(const dgll_csr_plan* plan, int heads, int fo);

/* out[k * heads + h] = the dropout multiplier for every nonzero k of a CSR and every head: fp32 [nnz, heads], exactly 0 or (float)(1 / (1 - p)).
 * The device and the host form evaluate the same function and agree bit for bit (the host form takes host pointers and needs no GPU).
 * For tests and for callers that want the mask as an array (the edge_scale of dgll_hip_gat_pass); training never calls them.          */
int dgll_hip_gat_dropout_mask(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads,
                              const uint32_t* seed, double p, float* out);
int dgll_host_gat_dropout_mask(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads, const uint32_t* seed,
                               double p, float* out);

/* ---- a10 / a4 as ONE launch: aggregate -> transform (bf16 storage, fp32 accumulation) ------------------------------------
 *   out[i, :] = act( A1[i, :K1] . W1 + reduce_{j in row i} X[j, :feat] . W2 + bias )
 * The MI355X form of the reference's only native kernel, relu(A.X.W) in one launch
 * (dgll/FusedKernel/gcn_fused_kernel.cu:5-74; A1 == NULL gives exactly that shape), and of sageConv's
 * act(src.W_s + mean(nbr).W_n) (sageconv.py:33-41,70-83): a workgroup gathers and reduces a tile of 32 destination rows
 * into LDS and feeds it to the MFMAs directly -- the aggregated matrix is never read back from HBM.
 *   Wt1 / Wt2     the TRANSPOSED weights, bf16, zero-padded to [w_rows >= 32 * ceil(N / 32), 64 * ceil(K / 64)] (ldw*: row
 *                 stride in elements).  Wt2 == NULL: the aggregate is ADDED to the output instead (feat == N) -- the
 *                 narrowing layer, whose neighbour product is aggregated after its transform;
 *   agg_out       optional [n_rows, ldagg] bf16: the aggregated rows (training keeps them for the weight gradient
 *                 agg^T . g).  REQUIRED when the plan has rows longer than its threshold: those are aggregated first by the
 *                 SpMM's chunk path into agg_out and loaded from there (workspace as for dgll_hip_spmm_csr);
 *   feat, N <= 256; X / A1 / out / agg_out rows 16-byte aligned; val NULL = unit edge values.                        */
int dgll_hip_sage_fused_forward(void* stream, const dgll_csr_plan* plan, const int64_t* rowptr, const int32_t* col,
                                const float* val, const void* X, int64_t ldx, int feat, int reduce,
                                const void* A1, int64_t lda1, int K1, const void* Wt1, int64_t ldw1,
                                const void* Wt2, int64_t ldw2, int w_rows, const float* bias, int relu, void* out,
                                int64_t ldo, int N, void* agg_out, int64_t ldagg, int64_t n_rows, int64_t n_cols,
                                void* workspace, size_t workspace_bytes);

/* ---- a3 (max): Y[i,f] = max_k X[col[k], f], arg[i,f] = the source row holding it (-1 / 0.0 for empty rows) --
 * NeighborAggregator's "max" (sageconv.py:37-38).  Y and arg share the leading dimension ldy; X/Y 16-byte
 * aligned with padded leading dimensions.                                                                   */
int dgll_hip_segment_max(void* stream, const int64_t* rowptr, const int32_t* col, const void* X, int64_t ldx,
                         void* Y, int32_t* arg, int64_t ldy, int dtype, int64_t n_rows, int feat);

/* Backward of the max: grad[j,f] = sum_{i lists j} (arg[i,f] == j) ? G[i,f] : 0  -- the gradient reaches the arg-max row
 * only (torch.max semantics behind sageconv.py:37-38).  (t_rowptr, t_col) is the TRANSPOSED structure (row j lists the
 * destination rows i in ascending order; a repeated pair counts once); one wavefront per output row, fixed order, no
 * atomics.  G / grad 16-byte aligned with leading dimensions padded like segment_max's; arg as segment_max wrote it. */
int dgll_hip_segment_max_bwd(void* stream, const int64_t* t_rowptr, const int32_t* t_col, const void* G, int64_t ldg,
                             const int32_t* arg, int64_t ldarg, void* grad, int64_t ldgrad, int dtype, int64_t n_src,
                             int feat);

/* ---- f2: feature-row gather through the hot-node cache -------------------------------------------------------
 * out[i,:] = cache[slot[idx[i]],:] if slot[idx[i]] >= 0 else host[idx[i],:]   -- GraphCacheServer.fetch_data,
 * dgll/FeatureCache/storage.py:151-198 (mask split, GPU gather of cached rows, CPU gather + copy of the rest, merge)
 * in one launch; `host` may be PINNED HOST memory (read over PCIe by the kernel) or a device matrix.  slot == NULL:
 * plain gather from `host` (dgll/data/dgraph.py:105 `features[nodes]`).  *miss_count (optional, device) is
 * incremented by the number of rows served from `host` (storage.py:213-220).                                 */
int dgll_hip_gather_rows(void* stream, const void* cache, int64_t ldc, const void* host, int64_t ldh,
                         const int64_t* idx, const int64_t* slot, void* out, int64_t ldo, int64_t n, int feat,
                         int dtype, unsigned long long* miss_count);

/* Same gather when the cache server holds a PARTITION of the graph: idx / slot are keyed by the partition-local id and
 * host_map[local id] is the row of `host` (the full-graph feature store) -- storage.py:27 `nid_map`, :104-107.  The
 * hit / miss split, both gathers and the miss count stay one launch; host_map == NULL is dgll_hip_gather_rows.      */
int dgll_hip_gather_rows_mapped(void* stream, const void* cache, int64_t ldc, const void* host, int64_t ldh,
                                const int64_t* idx, const int64_t* slot, const int64_t* host_map, void* out,
                                int64_t ldo, int64_t n, int feat, int dtype, unsigned long long* miss_count);

/* The reduction over a sampled block read STRAIGHT from the feature store:
 *   out[i,:] = reduce_{k in [rowptr[i], rowptr[i+1])} row(idx[k]),  row(v) = cache[slot[v],:] if slot[v] >= 0 else host[host_map[v] or v,:]
 * -- the K-axis mean of sageconv.py:33-36 over the outermost hop's neighbour features fused with GraphCacheServer.fetch_data
 * (storage.py:151-198): the fan-out x batch gathered rows are never materialised.  reduce: DGLL_REDUCE_SUM / _MEAN (empty rows: 0).
 * rowptr: int64 [n_rows + 1] over idx.  Rows must be 4-byte granular; 16-byte lanes are used when every pitch is a whole number of
 * 16-byte vectors (the padding columns are then summed and written as well).  *miss_count as in dgll_hip_gather_rows.            */
int dgll_hip_aggregate_rows_mapped(void* stream, const void* cache, int64_t ldc, const void* host, int64_t ldh,
                                   const int64_t* idx, const int64_t* slot, const int64_t* host_map, const int64_t* rowptr,
                                   void* out, int64_t ldo, int64_t n_rows, int feat, int dtype, int reduce,
                                   unsigned long long* miss_count);

/* The outermost hop of a natively sampled batch leaves the host as neighbour POSITIONS inside each seed's adjacency list
 * (dgll_host_sample_batch_seeded with defer_last; reference loop: base_sampler.py:45-58 keeps `neighbors[j]`, the lookup
 * `g.get_neighbors` is dgll/data/dgraph.py:49-62).  One launch turns them into node ids on the device:
 *     out_ids[k] = indices[ indptr[ seeds[r] ] + positions[k] ]      for k in [rowptr[r], rowptr[r + 1])
 * indptr / indices: the graph's CSR arrays in device memory (int64); seeds [n_rows] int64; rowptr [n_rows + 1] int64 (the hop's
 * row pointers: rowptr[r + 1] - rowptr[r] kept neighbours of seed r); positions: int16 / int32 / int64 entries (pos_bytes = 2, 4,
 * 8), rowptr[n_rows] of them.  Replaces five torch launches (gather of the starts, repeat_interleave, widening, add, gather). */
int dgll_hip_translate_positions(void* stream, const int64_t* indptr, const int64_t* indices, const int64_t* seeds,
                                 const int64_t* rowptr, int64_t n_rows, const void* positions, int pos_bytes, int64_t* out_ids);

/* Backward of the K-axis reduction over a SAMPLED block (sageconv.py:33-36 on a block whose source rows each belong to exactly one
 * destination row: col == arange(nnz), base_sampler.py:30-43 keeps duplicates): source row k of destination row r receives
 *     out[k, :] = scale_r * g[r, :]        scale_r = 1 / deg(r) for the mean (mean != 0), 1 for the sum,
 * k in [rowptr[r], rowptr[r + 1]); rows rowptr[n_rows] .. n_out_rows-1 of `out` (the unused tail of a block on static shapes) are
 * zeroed.  One launch instead of the degree / reciprocal / scale / searchsorted / gather chain of tensor ops (nine launches per
 * block and batch).  dtype: DGLL_F32 or DGLL_BF16 for both matrices (fp32 arithmetic); leading dimensions in elements.
 * accumulate != 0: out[k, :] += scale_r * g[r, :] instead (rows behind rowptr[n_rows] untouched): the rows already hold another
 * contribution to the same gradient (the layer's self path), written by an earlier launch.                                      */
int dgll_hip_expand_rows(void* stream, const int64_t* rowptr, int64_t n_rows, const void* g, int64_t ldg, void* out, int64_t ldo,
                         int64_t n_out_rows, int feat, int dtype, int mean, int accumulate);

/* The LOADING STAGE of one sampled mini-batch as ONE call (buffer_queues.py:22-46's `sample_generator` body: stage the batch on
 * the side stream; storage.py:151-198's fetch per hop; graphage.py:52-53's labels): everything the stage enqueues for a batch --
 *   1. the upload of the batch's staging buffer (seeds | source ids per hop | row pointers per hop: dgll_host_sample_batch_seeded's
 *      arrays at their upper-bound offsets) and of the outermost hop's neighbour positions, from pinned host memory,
 *   2. positions -> node ids of the outermost hop (dgll_hip_translate_positions),
 *   3. one cache gather per hop 0 .. n_hops-1 straight into that hop's rows of the consumer's input (dgll_hip_gather_rows_mapped),
 *   4. the outermost hop's reduction straight out of the cache (dgll_hip_aggregate_rows_mapped),
 *   5. the row pointers of hops 0 .. n_hops-2 padded to the consumer's static block shapes (entries past the batch's rows = its
 *      edge count: empty rows), and the seeds' labels (entries past the batch = label_fill) --
 * is issued on `stream` from native code: through Python the same work is ~15 launches and 1.0-1.8 ms of interpreter time per
 * batch on the loading thread, which bounds a pipeline whose GPU side takes 1.6 ms.  All pointers in device memory unless named
 * *_host (pinned).  Offsets are in int64 entries of the staging buffer.  rows[h] = rows of hop h (rows[h + 1] = edges of hop h);
 * n_outer = edges of the outermost hop.  miss_count: optional device counter (hit / miss accounting, storage.py:213-220).      */
typedef struct dgll_batch_load {
    const void* staged_host; int64_t staged_entries; int64_t* staged_dev;
    const void* pos_host; int64_t n_outer; int pos_bytes; void* pos_dev;
    const int64_t* indptr; const int64_t* indices;
    int n_hops; int64_t rows[8]; int64_t seeds_off; int64_t src_off[8]; int64_t ptr_off[8];
    const void* cache; int64_t ldc; const void* host; int64_t ldh; const int64_t* slot; const int64_t* host_map;
    int feat; int dtype; unsigned long long* miss_count;
    void* feat_out[8]; int64_t ld_feat;
    void* reduced_out; int64_t ld_reduced; int reduce;
    int64_t* ids_out;
    int64_t* rowptr_out[8]; int64_t rowptr_cap[8];
    const int64_t* labels; int64_t* labels_out; int64_t labels_cap; int64_t label_fill;
    /* Optional (stage_map NULL, or no slot map: the uncached rows of the outermost hop are read zero-copy by its reduction): fetch them
     * into HBM first -- every DISTINCT uncached node of the hop once, by a small grid that the link, not the CUs, bounds -- so that the
     * reduction reads HBM only and does not hold the chip while it waits for PCIe.  stage_map: int64[n_nodes] scratch of ONE loading
     * stream, zero-initialised once, never cleared (entries carry stage_serial, which the caller advances per call, never 0);
     * stage_rows: [stage_cap, ld_stage] elements of the store's dtype; stage_list: int64[stage_cap]; stage_count: one device word.
     * Nodes past stage_cap stay zero-copy reads.  stage_blocks: workgroups of the fetch (0 = about 192 KB of reads in flight: 20 at 1204-byte rows).                                   */
    int64_t* stage_map; void* stage_rows; int64_t ld_stage; int64_t stage_cap; int64_t* stage_list; unsigned int* stage_count;
    unsigned int stage_serial; int stage_blocks;
    int upload_blocks;      /* workgroups of the two uploads (0 = 16, DGLL_LOADER_UPLOAD_BLOCKS): few beside staged misses, more (128) when
                             * nothing else uses the link                                                                          */
} dgll_batch_load;
int dgll_hip_load_sampled_batch(void* stream, const dgll_batch_load* batch);

/* ---- f1 (host code): one hop of the reference's neighbour sampler, bit-exact with CPython 3.10's random.sample -------
 * For every seed in order: all neighbours if deg <= fanout (or fanout < 0), else random.sample(neighbors, fanout)
 * (/root/reference/dgll/sampling/base_sampler.py:45-58), drawn from the MT19937 state passed in (`random.getstate()`:
 * 624 words + index) and updated in place, so the ids and the generator stream are identical to the Python loop.
 * indptr/indices: CSR copy of DGraph.edges (HOST pointers, like every argument of this call).  `setsize` is
 * CPython's pool/set switch-over (21, or 21 + 4**ceil(log(3*fanout, 4)) when fanout > 5), computed by the caller.  */
int dgll_host_sample_neighbors(uint32_t* mt_state, int* mt_index, const int64_t* indptr, const int64_t* indices,
                               const int64_t* seeds, int64_t n_seeds, int64_t fanout, int64_t setsize,
                               int64_t* out_src, int64_t* out_dst, int64_t* out_counts, int64_t capacity, int64_t* n_out);
/* out_dst == NULL above stops after the (sequential) draw phase: out_src then holds POSITIONS inside each seed's adjacency
 * list.  This call finishes the job -- positions -> neighbour ids, out_dst = the seed of every edge -- and touches no
 * generator state, so a pipeline can run it on another thread while the next batch is being drawn.              */
int dgll_host_translate_neighbors(const int64_t* indptr, const int64_t* indices, const int64_t* seeds, int64_t n_seeds,
                                  const int64_t* counts, int64_t* src_inout, int64_t* out_dst);
/* random.seed(int) of CPython (init_by_array over `key` = the 32-bit little-endian words of abs(seed), [0] for 0) -> the 624-word
 * state and index (624) the calls above take: a sampler stream that lives OUTSIDE the interpreter's global generator.          */
int dgll_host_mt_seed(const uint32_t* key, int64_t key_len, uint32_t* mt_state, int* mt_index);
/* A whole mini-batch under its own seed: what the reference's loop (dgllsampler.py:10-21 over base_sampler.py:45-58) draws when
 * random.seed(seed) is called right before the batch.  Individually seeded batches are independent, so several host threads may
 * each draw whole batches concurrently, every one bit-identical to the reference loop under its seed (the reference's loop is
 * unseeded, base_sampler.py:56; its DataLoader-with-workers shape, MQGCN.py:114-128, gives every worker its own stream too).
 * Hops in SAMPLING order (reversed(fanouts)): hop h draws around the sources of hop h-1 (hop 0 around `seeds`), duplicates kept;
 * fanouts[h] < 0 = all neighbours; setsizes[h] as in dgll_host_sample_neighbors.  out_src/out_dst/out_counts: n_hops caller-owned
 * arrays of capacity[h] edges (counts: one per hop seed).  defer_last: the last hop keeps POSITIONS in out_src[h], out_dst[h] is
 * not written.  max_threads bounds the helper threads of the id translation inside this call.                                  */
int dgll_host_sample_batch_seeded(const uint32_t* key, int64_t key_len, const int64_t* indptr, const int64_t* indices,
                                  const int64_t* seeds, int64_t n_seeds, const int64_t* fanouts, const int64_t* setsizes, int n_hops,
                                  int64_t* const* out_src, int64_t* const* out_dst, int64_t* const* out_counts,
                                  const int64_t* capacity, int64_t* n_out, int defer_last, int max_threads);

/* ---- f1 / f2 (host code): a pool of native sampler threads behind one in-order hand-over -- the first of the reference's three
 * queues (README.md:27-29; buffer_queues.py:22-46's sample_generator) without an interpreter in the producers.  `n_threads` workers
 * draw the batches of one epoch -- batch i = train_nodes[i * batch_size, (i + 1) * batch_size), under
 * random.seed((base_seed << 40) | (epoch << 20) | i): exactly dgll_host_sample_batch_seeded's ids (outermost hop left as positions) --
 * each into slot i % n_slots of caller-owned (pinned) buffers:
 *   staged_bufs[slot]  int64[staged_entries]: seeds at off_seeds, the source ids of hop h < n_hops - 1 at off_src[h], the row pointers
 *                      of hop h (rows + 1 prefix sums of the kept-neighbour counts) at off_ptr[h] -- ONE upload for the loading stage;
 *   pos_bufs[slot]     the outermost hop's neighbour POSITIONS as pos_bytes-byte (2 / 4 / 8) unsigned integers.
 * fanouts / setsizes in SAMPLING order (the reference's reversed(fanouts)), setsizes as for dgll_host_sample_neighbors.
 * n_slots >= n_threads + 1; base_seed < 2**24, epoch and the batch count < 2**20 (the seed is one 64-bit word).
 * _next: the next batch IN ORDER, blocking: 0 = out[0] batch, out[1] slot, out[2] n_hops, out[3 ..) rows per hop, then edges per hop;
 *        1 = epoch over; < 0 = a worker failed.  ONE consumer thread.   _release: the slot's uploads are complete, it may be rewritten.
 * _destroy: stops and joins the workers.  Threading: the pool's own; the adjacency arrays are read-only and shared.               */
typedef struct dgll_sampler_pool dgll_sampler_pool;
int dgll_host_sampler_pool_create(dgll_sampler_pool** out, const int64_t* indptr, const int64_t* indices, const int64_t* train_nodes,
                                  int64_t n_train, int64_t batch_size, const int64_t* fanouts, const int64_t* setsizes, int n_hops,
                                  uint64_t base_seed, uint64_t epoch, int n_threads, int n_slots, int64_t* const* staged_bufs,
                                  int64_t staged_entries, int64_t off_seeds, const int64_t* off_src, const int64_t* off_ptr,
                                  void* const* pos_bufs, int pos_bytes);
int dgll_host_sampler_pool_next(dgll_sampler_pool* pool, int64_t* out, double* sample_ms);
int dgll_host_sampler_pool_release(dgll_sampler_pool* pool, int slot);
int dgll_host_sampler_pool_destroy(dgll_sampler_pool* pool);

/* ---- the optimizer step of the training loops as ONE launch (torch.optim.Adam's arithmetic; MQGCN.py:141-144, train_gcn.py:26) --
 * Adam over a flat fp32 parameter buffer: param/grad/exp_avg/exp_avg_sq [n]; `step` = 1, 2, ... (bias corrections formed in double
 * on the host); grad_scale multiplies the gradient first (1 / world_size of the RaCoM average, MQGCN.py:64).  Segments (optional,
 * at most 24): element range [seg_begin, seg_end) is a [rows, seg_cols] weight matrix whose updated values are ALSO written, as
 * bf16, into seg_packed ([rows, seg_ld], W itself) and seg_packed_t ([cols, seg_ldt], W transposed) -- the zero-padded forms
 * dgll_hip_transform_bf16 takes (what dgll_hip_pack_weight_bf16 produces per product otherwise); either pointer may be NULL.   */
int dgll_hip_adam_flat(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale, int n_segments,
                       const int64_t* seg_begin, const int64_t* seg_end, const int* seg_cols, void* const* seg_packed,
                       const int64_t* seg_ld, void* const* seg_packed_t, const int64_t* seg_ldt);

/* ---- dense transform, exact fp32: C[M,N] = act(A[M,K].B[K,N] + bias) --------------------------------------
 * F.mm / F.matmul of gcnconv.py:30, sageconv.py:41,72, gatconv.py:31,117 for callers that only have the C ABI
 * (fmaf accumulation in k order: bit-stable).  relu != 0 fuses max(.,0); bias may be NULL.                   */
int dgll_hip_gemm_f32(void* stream, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                      int64_t M, int N, int K, const float* bias, int relu);

/* ---- fp32 dense products on the matrix cores (the 1e-4 parity path of the layers) -------------------------------------------
 * dgll_hip_mm_f32:  C[M, N] = act(A[M, K] . Wt[N, K]^T + addend + bias), everything fp32, v_mfma_f32_32x32x2_f32 (fp32 inputs, fp32
 * accumulation: exact fp32 FMA arithmetic).  Wt is the weight TRANSPOSED ([N, K] row-major; for an input gradient g . W^T pass
 * Wt := W).  N <= 256 per call (split columns on the host); any alignment (16-byte aligned rows take float4 loads).
 * dgll_hip_mm2_f32:  C = gate(act(A1 . W1t^T + A2 . W2t^T + addend + bias)): sageConv's self + neighbour term (sageconv.py:72-75), or
 * a layer's two input-gradient products, in ONE accumulation; A2 may be NULL (then W2t / K2 are ignored); gate (optional, [M, ldgate]):
 * outputs are zeroed where gate <= 0 -- the ReLU mask of the layer below applied by the epilogue.  N <= 256 per call.
 * dgll_hip_grad_weight_f32:  dW[K, N] = X[M, K]^T . G[M, N] on the same instruction: the long reduction is split over `slabs` row
 * slabs (rows summed in order inside a slab) whose partials (workspace: dgll_hip_grad_weight_f32_workspace bytes) are summed in
 * slab order -- deterministic, no atomics.                                                                                  */
int dgll_hip_mm_f32(void* stream, const float* A, int64_t lda, const float* Wt, int64_t ldw, float* C, int64_t ldc,
                    int64_t M, int N, int K, const float* bias, int relu, const float* addend, int64_t ldadd);
int dgll_hip_mm2_f32(void* stream, const float* A1, int64_t lda1, const float* W1t, int64_t ldw1, int K1, const float* A2,
                     int64_t lda2, const float* W2t, int64_t ldw2, int K2, float* C, int64_t ldc, int64_t M, int N,
                     const float* bias, int relu, const float* addend, int64_t ldadd, const float* gate, int64_t ldgate);
int64_t dgll_hip_grad_weight_f32_workspace(int K, int N, int slabs);
int dgll_hip_grad_weight_f32(void* stream, const float* X, int64_t ldx, const float* G, int64_t ldg, float* dW,
                             int64_t lddw, int64_t M, int K, int N, void* workspace, int64_t workspace_bytes, int slabs);

/* Wt operand of the transforms from a parameter: dst[r, c] = bf16(src[r*stride_row + c*stride_col]) for r < n, c < k, zero
 * elsewhere, dst bf16 [rows >= n, ld >= k].  src fp32 or bf16, any element strides (pass a [K, N] parameter as its transposed view:
 * stride_row = 1, stride_col = N) -- the cast, the zero padding and the layout in one launch.                                    */
int dgll_hip_pack_weight_bf16(void* stream, const void* src, int src_dtype, int64_t stride_row, int64_t stride_col, int n, int k,
                              void* dst, int64_t ld, int rows);
/* ---- bf16 MFMA transform: out[M,N] = act( A1[M,K1].Wt1[N,K1]^T (+ A2[M,K2].Wt2[N,K2]^T) + bias ) -------------
 * The dense W-transform next to the aggregation on matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulation):
 * sageConv's act(src.W_s + agg.W_n) in ONE pass (sageconv.py:71-82), gcnConv / GAT x.W (gcnconv.py:30,
 * gatconv.py:31,117), and their input gradients g.W^T (pass Wt := W; `relu_mask`, same shape as A1, fuses the
 * ReLU backward: A1 is zeroed where the mask is <= 0).  A*: bf16 row-major, 16-byte aligned, lda a multiple of 8.
 * Wt*: the weight TRANSPOSED, bf16, zero padded to [64 rows if N <= 64, 128 if N <= 128, else 256] x
 * [ld >= 64*ceil(K/64) columns] (the kernel stages 2, 4 or 8 column tiles of 32 rows of Wt).  N <= 256.
 * out: bf16 or fp32 [M, ldo].  A2/Wt2/relu_mask/bias may be NULL.
 * relu: bit 0 = fuse max(., 0); bit 1 (bf16 output, ldo a multiple of 8, 16-byte aligned) = the row padding [N, ldo)
 * belongs to the output and is written with zeros: rows are stored as whole 16-byte vectors / whole lines (a 47-column
 * row on a 128-byte pitch: 256 -> 47 runs at the speed of 256 -> 64 instead of 25 % slower).                         */
int dgll_hip_transform_bf16(void* stream, const void* A1, int64_t lda1, int K1, const void* Wt1, int64_t ldw1,
                            const void* A2, int64_t lda2, int K2, const void* Wt2, int64_t ldw2, int wt_rows,
                            const void* relu_mask, int64_t ldm, void* out, int64_t ldo, int out_dtype,
                            int64_t M, int N, int relu, const float* bias);   /* wt_rows: rows allocated in Wt1/Wt2 */
/* The same with an OUTPUT gate: out[i, n] is written as 0 where out_gate[i, n] <= 0 (bf16 [M, ldgate], may be NULL) --
 * the input gradient g.Ws^T + gz.Wn^T of a layer whose input came out of a ReLU, masked in the epilogue -- and an
 * optional per-row factor (fp32 [M], may be NULL): out = act(row_scale[i] * (A.W) + bias), e.g. the 1/deg of a mean
 * aggregation folded into the product that is aggregated next, so that SpMM runs unweighted.                       */
int dgll_hip_transform_bf16_gated(void* stream, const void* A1, int64_t lda1, int K1, const void* Wt1, int64_t ldw1,
                                  const void* A2, int64_t lda2, int K2, const void* Wt2, int64_t ldw2, int wt_rows,
                                  const void* relu_mask, int64_t ldm, void* out, int64_t ldo, int out_dtype,
                                  int64_t M, int N, int relu, const float* bias, const void* out_gate, int64_t ldgate,
                                  const float* row_scale);

/* The same transform with a bf16 [M, ldadd] matrix added before the activation:
 * out = act(row_scale * (A1.Wt1^T + A2.Wt2^T) + bias + addend) -- the self term of a transform-first SAGE layer, whose
 * neighbour term arrives already aggregated (sageconv.py:72-75 computes src.W + aggregated as two ops and an add). */
int dgll_hip_transform_bf16_add(void* stream, const void* A1, int64_t lda1, int K1, const void* Wt1, int64_t ldw1,
                                const void* A2, int64_t lda2, int K2, const void* Wt2, int64_t ldw2, int wt_rows,
                                const void* relu_mask, int64_t ldm, void* out, int64_t ldo, int out_dtype, int64_t M,
                                int N, int relu, const float* bias, const void* out_gate, int64_t ldgate,
                                const float* row_scale, const void* addend, int64_t ldadd);

/* The transform with the ReLU gate carried as ONE BIT PER ELEMENT instead of a bf16 matrix (bf16 output; no input mask, row
 * scale or addend).  The reference keeps the activation itself for autograd's ReLU backward (models/sage.py applies F.relu between
 * sageConv layers; sageconv.py:72-82 the in-layer activation): 512 bytes of a 256-column row are read back only to learn 256 signs.
 *   bits_out (may be NULL): uint32 [M, ld_bits_out]; word w of row i, bit b <- out[i, 32 w + b] > 0, from the values the epilogue
 *     stores (stores only: the producing transform is no slower); words up to 4 * ceil(N / 128) are written, zero past N;
 *   gate_bits (may be NULL): such a matrix, read INSTEAD of out_gate: out[i, n] is written as 0 where its bit is clear.  The
 *     resident-weights kernel fetches a block's words one reduction phase ahead of its epilogue; shapes that run the 4-wave
 *     kernel read out_gate (pass both; gate_bits alone is an error there).  Both describe the same gate: out_gate[i, n] > 0.
 * ld_*: words per row, multiples of 4, >= 4 * ceil(N / 128); 16-byte aligned bases.  Other arguments as dgll_hip_transform_bf16. */
int dgll_hip_transform_bf16_bits(void* stream, const void* A1, int64_t lda1, int K1, const void* Wt1, int64_t ldw1,
                                 const void* A2, int64_t lda2, int K2, const void* Wt2, int64_t ldw2, int wt_rows,
                                 void* out, int64_t ldo, int64_t M, int N, int relu, const float* bias,
                                 const void* out_gate, int64_t ldgate, const uint32_t* gate_bits, int64_t ld_gate_bits,
                                 uint32_t* bits_out, int64_t ld_bits_out);

/* Two products of ONE activation matrix: out1 = A.Wt1^T and out2 = A.Wt2^T, A read once -- the two input gradients
 * g.Ws^T and g.Wn^T of a SAGE layer (what autograd derives for sageconv.py:72-75's `src @ W` pair).  bf16 A [M, lda],
 * Wt1 / Wt2 [wt_rows >= 256, ldw] zero-padded as dgll_hip_transform_bf16 wants them, bf16 out1 / out2 [M, ldo >= N];
 * K, N <= 256.                                                                                                      */
int dgll_hip_transform_bf16_dual(void* stream, const void* A, int64_t lda, int K, const void* Wt1, const void* Wt2,
                                 int64_t ldw, int wt_rows, void* out1, int64_t ldo1, void* out2, int64_t ldo2, int64_t M,
                                 int N);

/* ---- weight gradients of the dense transform: dW1 = X1^T . G and (optionally) dW2 = X2^T . G ---------------------
 * What autograd derives for `self.W(h)` / `neigh @ self.W` (sageconv.py:41,72-75; gcnconv.py:30; the reference leaves it
 * to two library GEMMs that each read G).  bf16 X1 [M, ldx1 >= K1], X2 [M, ldx2 >= K2] (NULL / K2 = 0: one product),
 * G [M, ldg >= N]; fp32 dW1 [K1, lddw1 >= N], dW2 [K2, lddw2 >= N]; K1, K2, N <= 256; rows 16-byte aligned (bases, and leading
 * dimensions multiples of 8).  Split over `n_slabs` row slabs (1..4096) whose partials are summed in slab order (deterministic);
 * `workspace`: dgll_hip_grad_weight_workspace(K1, K2, n_slabs) bytes of device memory.  M = 0 (inputs may be NULL) writes zeros.      */
int64_t dgll_hip_grad_weight_workspace(int K1, int K2, int n_slabs);
int dgll_hip_grad_weight_bf16(void* stream, const void* X1, int64_t ldx1, int K1, const void* X2, int64_t ldx2, int K2,
                              const void* G, int64_t ldg, int N, int64_t M, void* workspace, int64_t workspace_bytes,
                              int n_slabs, float* dW1, int64_t lddw1, float* dW2, int64_t lddw2);
/* The same launch with both results stored transposed: dW1 [N, lddw1 >= K1] = G^T . X1, dW2 [N, lddw2 >= K2] = G^T . X2.  Called with
 * X1 = g, X2 = A^T g, G = h it yields dWs = h^T . g and dWn = h^T . (A^T g) of the narrowing SAGE layer (sageconv.py:72-82 with the
 * narrow product aggregated) with the wide operand h read once for both.                                                          */
int dgll_hip_grad_weight_bf16_tr(void* stream, const void* X1, int64_t ldx1, int K1, const void* X2, int64_t ldx2, int K2,
                                 const void* G, int64_t ldg, int N, int64_t M, void* workspace, int64_t workspace_bytes,
                                 int n_slabs, float* dW1, int64_t lddw1, float* dW2, int64_t lddw2);

/* ---- the loss at the end of the path: softmax cross-entropy with class-index targets ---------------------------
 * nn.CrossEntropyLoss on the last layer's output (Evaluation/PPI/train_gcn.py:27,45), one pass per direction:
 * row_loss[i] = logsumexp(z_i) - z_i[label_i]  and/or  grad[i, c] = *grad_scale * (softmax(z_i)[c] - [c == label_i]).
 * logits/grad: fp32 or bf16 [n_rows, ld]; labels int64, a label outside [0, n_classes) (e.g. -100) is ignored (loss 0,
 * zero gradient); grad_scale: DEVICE pointer to one float (NULL = 1), so upstream gradients need no host sync.
 * row_loss or grad may be NULL.  n_classes <= 1024.                                                              */
int dgll_hip_softmax_xent(void* stream, const void* logits, int64_t ldz, int dtype, const int64_t* labels,
                          float* row_loss, void* grad, int64_t ldg, const float* grad_scale, int64_t n_rows,
                          int n_classes);
/* The same loss with probability / multi-hot targets (fp32 [n_rows, ldt]) -- what nn.CrossEntropyLoss computes for the
 * float label matrix of the PPI loop (train_gcn.py:27,45): row_loss[i] = -sum_c t_ic log softmax(z_i)[c],
 * grad[i, c] = *grad_scale * (softmax(z_i)[c] * sum_c t_ic - t_ic).                                             */
int dgll_hip_softmax_xent_soft(void* stream, const void* logits, int64_t ldz, int dtype, const float* targets,
                               int64_t ldt, float* row_loss, void* grad, int64_t ldg, const float* grad_scale,
                               int64_t n_rows, int n_classes);
/* Both target kinds behind one entry (exactly one of labels / targets non-NULL) + flags.  bit 0: the logits are ReLU outputs and
 * the gradient returned is d loss / d PRE-activation: zero wherever the logit is <= 0 (the last sageConv's ReLU backward,
 * sageconv.py:83, folded into the loss's gradient pass instead of a separate pass over [n_rows, n_classes]).  bit 1: the padding
 * [n_classes, ldg) of the gradient rows belongs to the output and may be written with zeros (whole 16-byte stores).            */
int dgll_hip_softmax_xent_ex(void* stream, const void* logits, int64_t ldz, int dtype, const int64_t* labels, const float* targets,
                             int64_t ldt, float* row_loss, void* grad, int64_t ldg, const float* grad_scale, int64_t n_rows,
                             int n_classes, int flags);
/* The loss of a (mini-)batch out of its per-row losses in ONE launch: out4 = {sum of row_loss, number of labels in [0, n_classes)
 * (labels NULL: n_rows), their quotient -- nn.CrossEntropyLoss(reduction='mean'), train_gcn.py:27 / buffer_queues.py:106 --, 1 / count (the
 * scale of the gradient pass)}.  One workgroup, fixed summation order; n_rows <= 2^20.                                          */
int dgll_hip_xent_reduce(void* stream, const float* row_loss, const int64_t* labels, int64_t n_rows, int n_classes, float* out4);


/* ---- layer-wise importance sampling (LADIES / FastGCN; dgll_amd/sampling/layerwise.py) -------------------------------------
 * L is a CSR (int64 rowptr, int32 col, fp32 val or NULL = 1) over n_total nodes; rows (int64) select its rows (NULL: all).
 * info: int64[8] per layer, {candidates, s, columns of the block, nnz, error bits}; the host reads it once per layer.
 * marker / mark: uint32[n_total] epoch tags (start zeroed, never cleared: every use passes a fresh non-zero epoch).
 * Column mass: mass[c] = sum_{rows} rint(val^2 * 2^shift) (integer atomics, bitwise reproducible); cand (int32[n_total]) lists the
 * distinct touched columns, their number in info[0]; totals = {sum of high halves, sum of low halves} of q (q = mass, or with
 * flat sqrt(mass) in 2^-40 units).  Zeroes info[0..7] and totals first.  seg: int64[n_rows + 1] workspace (the rows' entry
 * offsets: every pass over the entries is flat, whatever the row lengths; unused when rows is NULL).                         */
int dgll_hip_lw_column_mass(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, const int64_t* rows,
                            int64_t n_rows, int64_t n_total, uint32_t* marker, uint32_t epoch, unsigned long long* mass,
                            int shift, int flat, int32_t* cand, int64_t* info, unsigned long long* totals, int64_t* seg);
/* p[i] = q(ids[i]) / sum q, for i < min(*count, cap) (count NULL: cap); fp64.                                                  */
int dgll_hip_lw_column_p(void* stream, const int64_t* ids, const int64_t* count, int64_t cap, const unsigned long long* mass,
                         int shift, int flat, const unsigned long long* totals, double* p);
/* Words of the select's ctrl workspace (unsigned long long).                                                                   */
int64_t dgll_hip_lw_ctrl_words(void);
/* s = min(#{q > 0}, fanout) of the *cand_count candidates drawn without replacement with probability q / sum q, in draw order,
 * into out_ids[0..s) (int64); s into info[1] and info[2].  Keys E / q, E = -log U, U from Philox4x32-10 with key = seed and
 * counter = (node, 0, layer, const): a node's key depends on (seed, layer, node, q) only.  Workspaces: keys[cand_cap],
 * ctrl[dgll_hip_lw_ctrl_words()], win_key / win_id [win_cap >= fanout].                                                        */
int dgll_hip_lw_select(void* stream, const int32_t* cand, const int64_t* cand_count, int64_t cand_cap, const unsigned long long* mass,
                       int shift, int flat, uint64_t seed, int layer, int64_t fanout, unsigned long long* keys, unsigned long long* ctrl,
                       unsigned long long* win_key, int32_t* win_id, int64_t win_cap, int64_t* out_ids, int64_t* info);
/* out = sorted unique(a[0..min(*a_count, a_cap)) u b[0..nb)), its length into info[2].  reps / out: a_cap + nb entries.         */
int dgll_hip_lw_union_sorted(void* stream, const int64_t* a, const int64_t* a_count, int64_t a_cap, const int64_t* b, int64_t nb,
                             int64_t n_total, uint32_t* marker, uint32_t epoch, int64_t* reps, unsigned long long* n_reps,
                             int64_t* out, int64_t* info);
/* Weights of m = min(*m_dev, cap) (m_dev NULL: cap) columns with probabilities p (draw order), fp64.  mode 0: the reference's
 * estWRS_weights with n = n_total; mode 1: 1 / (p * s), s = *snum_dev (NULL: snum).  One workgroup.                            */
int dgll_hip_lw_weights(void* stream, const double* p, const int64_t* m_dev, int64_t cap, const int64_t* snum_dev, int64_t snum,
                        int64_t n_total, int mode, double* w);
/* Block L[rows, cols] -- structure: maps cols (local id = position) through mark / local, counts the kept entries of every row
 * and scans them into out_rowptr (int64[n_rows + 1]); nnz into info[3].  sorted: cols ascend (CSR order is local order), a
 * wavefront per row.  Otherwise m_cap <= 4096 and the passes are flat over the entries: seg int64[n_rows + 1], bitmap uint32 and
 * below int32 [n_rows * 128] workspaces, kept for dgll_hip_lw_block_fill.                                                    */
int dgll_hip_lw_block_count(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* rows, int64_t n_rows,
                            int64_t n_total, const int64_t* cols, const int64_t* m_dev, int64_t m_cap, uint32_t* mark,
                            int32_t* local, uint32_t epoch, int sorted, int64_t* seg, uint32_t* bitmap, int32_t* below,
                            int64_t* out_rowptr, int64_t* info);
/* ... and values: out_col (int32 local ids, ascending within a row), out_val = val * w[local]; the same sorted flag and
 * workspaces as the count.                                                                                                     */
int dgll_hip_lw_block_fill(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, const int64_t* rows,
                           int64_t n_rows, int64_t n_total, const uint32_t* mark, const int32_t* local, uint32_t epoch,
                           const double* w, int sorted, int64_t m, const int64_t* seg, const uint32_t* bitmap, const int32_t* below,
                           const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* info);
/* Philox4x32-10 of one counter (host; the samplers' generator, for tests).                                                     */
int dgll_host_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4);


/* ---- neighbour sampling into message-flow-graph blocks (dgll_amd/sampling/neighbor.py) --------------------------------------
 * The graph is a CSR of in-neighbours (int64 rowptr, int32 col) over n_total < 2^31 nodes, every row shorter than 2^32; rows
 * (int64[n_rows], distinct) are the destinations of one layer.  Destination row r with id v and degree d keeps all d entries when
 * fanout == -1 or d <= fanout, otherwise `fanout` distinct positions of v's adjacency list, every subset equally likely, by
 * Floyd's algorithm: for i = 0 .. fanout-1, j = d - fanout + i, t = mulhi32(word_i, j + 1), take t unless taken, else j; word_i is
 * word i % 4 of Philox4x32-10 with key = {seed lo, seed hi} and counter = {v lo, v hi, layer, i / 4}.  The draw of (seed, layer, v,
 * fanout) depends on nothing else.  Kept entries stay in ascending position.
 * Workspaces that persist per graph: mark uint32[n_total] (epoch tags: start zeroed, never cleared, every call passes a fresh
 * non-zero epoch), local int32[n_total]; per call: bitmap uint32[ceil(n_total / 32)] (cleared here), prefix int32[the same],
 * drawn int32[drawn_cap >= n_rows * fanout] (unused and may be NULL when fanout == -1: the entries are the graph's own).
 * Outputs: out_rowptr int64[n_rows + 1]; info int64[8] (zeroed here) = {nnz, number of drawn nodes that are no destination, error
 * bits: 1 a row id outside [0, n_total), 2 a column id outside it, 4 a destination listed twice}.  The caller reads info once,
 * sizes the outputs and calls dgll_hip_nb_block with the same workspaces and epoch.                                              */
int dgll_hip_nb_sample(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, const int64_t* rows, int64_t n_rows,
                       int fanout, uint64_t seed, int layer, uint32_t* mark, int32_t* local, uint32_t epoch, uint32_t* bitmap,
                       int32_t* prefix, int32_t* drawn, int64_t drawn_cap, int64_t* out_rowptr, int64_t* info);
/* The block of that draw: src_nodes int64[n_rows + n_new] = [rows in their order | the new ids ascending]; out_col int32[nnz] local
 * ids into src_nodes, ascending within a row; out_val fp32[nnz] = 1 / (entries of the row), or NULL for none.  loc: int32[nnz]
 * workspace.  Only after info[2] == 0.                                                                                          */
int dgll_hip_nb_block(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, const int64_t* rows, int64_t n_rows,
                      int fanout, const uint32_t* mark, const int32_t* local, uint32_t epoch, const uint32_t* bitmap,
                      const int32_t* prefix, const int32_t* drawn, const int64_t* out_rowptr, int64_t nnz, int64_t n_new,
                      int32_t* loc, int64_t* src_nodes, int32_t* out_col, float* out_val);
/* The largest fan-out dgll_hip_nb_sample draws (64: one kept position per lane of a wavefront).                                  */
int dgll_hip_nb_max_fanout(void);
/* dgll_hip_nb_sample with an edge-weighted draw: weight fp32[nnz], one positive finite weight per entry of the graph (entries of
 * weight 0 are removed by the caller beforehand).  fanout in [1, 64] only.  A row of degree d <= fanout is copied; otherwise
 * position p of node v's row gets key = -log(u) / (double)weight in fp64, u = (bits + 0.5) * 2^-53, bits = ((x0 << 32) | x1) >> 11 of
 * ONE Philox4x32-10 call with key = {seed lo, seed hi} and counter = {v lo, v hi, layer | 0x80000000, p}, and the `fanout` smallest
 * by (key bits as uint64, position) are kept: successive draws without replacement in proportion to the weights.  Same outputs,
 * workspaces and info as dgll_hip_nb_sample, then dgll_hip_nb_block with the same fanout; drawn: int32[drawn_cap],
 * drawn_cap >= n_rows * (fanout + 1) (the last n_rows entries list the rows longer than dgll_hip_nb_long_row()).  info[2] bit 8: a
 * weight that is no positive finite number was met (it is never selected).                                                      */
int dgll_hip_nb_sample_weighted(void* stream, const int64_t* rowptr, const int32_t* col, const float* weight, int64_t n_total,
                                const int64_t* rows, int64_t n_rows, int fanout, uint64_t seed, int layer, uint32_t* mark, int32_t* local,
                                uint32_t epoch, uint32_t* bitmap, int32_t* prefix, int32_t* drawn, int64_t drawn_cap, int64_t* out_rowptr,
                                int64_t* info);
/* Rows of more entries than this are drawn by a workgroup each, shorter ones by a lane group (dgll_hip_nb_sample_weighted).      */
int dgll_hip_nb_long_row(void);

/* ---- link prediction: edge batches, negatives, exclusion, pair scores (dgll_amd/sampling/edge.py, dgll_amd/ops_pair.py) -------
 * The graph is the neighbour sampler's CSR of in-neighbours over n_total < 2^31 nodes with nnz entries; entry e of row v is the edge
 * col[e] -> v and e is its edge id.  edge_ids int64[n_edges] (duplicates allowed) is one batch; K = negatives >= 0.
 * pairs int32[pairs_cap >= n_edges * (1 + K), 2] receives GLOBAL (src, dst) ids: row i < n_edges is positive i, (col[e], the row
 * of e); row n_edges + i * K + k is negative k of positive i, (col[e], c).  c comes from attempts a = 0, 1, ...:
 * c = mulhi32(x[0], n_total), x = Philox4x32-10 with key = {seed lo, seed hi} and counter = {e lo, e hi, k | 0x40000000, a} (a
 * domain apart from the neighbour sampler's layer and layer | 0x80000000: one seed may drive both).  filter_existing == 0: attempt
 * 0 is taken.  Otherwise c is rejected while col[e] occurs in row c (binary search: columns ascending within every row), and
 * after max_attempts >= 1 rejections the last candidate is kept and counted.  A negative depends on (seed, e, k) only.
 * Workspaces: mark uint32[n_total] persists per graph (epoch tags: start zeroed, never cleared, a fresh non-zero epoch per call);
 * bitmap uint32[ceil(n_total / 32)] (cleared here) receives the bit of every endpoint, prefix int32[the same] the set bits below
 * each word.  info int64[8] (zeroed here) = {distinct endpoints M, capped negatives, error bits: 1 an edge id outside [0, nnz),
 * 2 a column id outside [0, n_total)}.  The caller reads info once, sizes the outputs and calls dgll_hip_ep_compact.            */
int dgll_hip_ep_draw(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, const int64_t* edge_ids,
                     int64_t n_edges, int negatives, int filter_existing, int max_attempts, uint64_t seed, uint32_t* mark, uint32_t epoch,
                     uint32_t* bitmap, int32_t* prefix, int32_t* pairs, int64_t pairs_cap, int64_t* info);
/* output_nodes int64[n_nodes = M]: the distinct endpoints in ascending id order; local_pairs int32[n_pairs, 2]: `pairs` as
 * positions in output_nodes.  Only after info[2] == 0.                                                                          */
int dgll_hip_ep_compact(void* stream, int64_t n_total, const uint32_t* bitmap, const int32_t* prefix, int64_t n_nodes,
                        const int32_t* pairs, int64_t n_pairs, int64_t* output_nodes, int32_t* local_pairs);
/* Remove from a block (int64 rowptr[n_rows + 1], int32 local col[nnz]; src_nodes int64[n_cols] its sources' global ids, the first
 * n_rows of them its destinations) every entry a -> b whose key b * n_total + a is in keys int64[n_keys > 0], sorted ascending.
 * _count: out_rowptr int64[n_rows + 1] = row pointers of the kept entries, info[0] = their number.  _fill (same arguments, that
 * out_rowptr, out_nnz = info[0]): out_col int32[out_nnz] the kept entries in their order, out_val fp32[out_nnz] = 1 / (kept
 * entries of the row) or NULL for none.                                                                                         */
int dgll_hip_ep_exclude_count(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t nnz, const int64_t* src_nodes,
                              int64_t n_cols, int64_t n_total, const int64_t* keys, int64_t n_keys, int64_t* out_rowptr, int64_t* info);
int dgll_hip_ep_exclude_fill(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t nnz, const int64_t* src_nodes,
                             int64_t n_cols, int64_t n_total, const int64_t* keys, int64_t n_keys, const int64_t* out_rowptr, int64_t out_nnz,
                             int32_t* out_col, float* out_val);
/* score[p] = <h[pairs[p, 0]], h[pairs[p, 1]]> in fp32.  h: [n_nodes, feat] of `dtype`, base 16-byte aligned, ldh (elements) a
 * whole number of 16-byte vectors >= feat; the padding of a row may hold anything.  A pair with an id outside [0, n_nodes) scores
 * NaN and reads nothing.                                                                                                       */
int dgll_hip_pair_dot(void* stream, const void* h, int64_t ldh, int64_t n_nodes, int feat, int dtype, const int32_t* pairs, int64_t n_pairs,
                      float* score);
/* grad_h[i] = sum over e in [inc_rowptr[i], inc_rowptr[i + 1]), in that order, of g[inc_pair[e]] * h[inc_other[e]]: fp32
 * accumulation, no atomics, written in `dtype` (rows without entries: zeros).  The incidence CSR lists, for node i, every pair
 * slot that holds i with the pair's other endpoint, ascending by (pair, slot).  grad_h: ldg (elements) a whole number of 16-byte
 * vectors covering feat rounded up to one; the padding columns are written (zeros).                                             */
int dgll_hip_pair_dot_bwd(void* stream, const void* h, int64_t ldh, int64_t n_nodes, int feat, int dtype, const int64_t* inc_rowptr,
                          const int32_t* inc_pair, const int32_t* inc_other, int64_t n_pairs, const float* g, void* grad_h, int64_t ldg);

/* ---- induced subgraphs and GraphSAINT node sets (dgll_amd/sampling/subgraph.py) ------------------------------------------------
 * The parent is a square CSR over n_total < 2^31 nodes with nnz entries (int64 rowptr, int32 col, optional fp32 val); its rows need
 * not be sorted and may hold parallel entries.  nodes int64[m] (distinct, any order) lists the subgraph's nodes: output row i is
 * parent row nodes[i] restricted to the entries whose column is listed, in the parent's order, each column rewritten to its
 * position in `nodes`.
 * Workspace that persists per graph: tag uint64[n_total], epoch << 32 | local id (starts zeroed, never cleared, every call passes a
 * fresh non-zero epoch).  dgll_hip_sg_count marks the nodes (64-bit atomic exchange), counts the kept entries of every row and scans:
 * out_rowptr int64[m + 1]; info int64[8] (zeroed here) = {nnz of the subgraph, -, error bits: 1 a node id outside [0, n_total),
 * 2 a column id outside it, 4 a node listed twice}.  The caller reads info once, sizes the outputs and calls dgll_hip_sg_fill with the
 * same tags and epoch.  m == 0 is allowed (out_rowptr = {0}).                                                                    */
int dgll_hip_sg_count(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, const int64_t* nodes, int64_t m,
                      uint64_t* tag, uint32_t epoch, int64_t* out_rowptr, int64_t* info);
/* The entries of that subgraph (out_nnz = info[0]): out_col int32[out_nnz] local ids; out_val fp32[out_nnz] or NULL for none: the
 * parent's value of the entry when val is given, 1 / (kept entries of the row) when val is NULL; out_eid int64[out_nnz] or NULL:
 * the parent's entry index of every kept entry.  The kept entries of a row keep the parent's order; two runs give the same bits.
 * Only after info[2] == 0.                                                                                                       */
int dgll_hip_sg_fill(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_total, int64_t nnz,
                     const int64_t* nodes, int64_t m, const uint64_t* tag, uint32_t epoch, const int64_t* out_rowptr, int64_t out_nnz,
                     int32_t* out_col, float* out_val, int64_t* out_eid, int64_t* info);
/* Rows of more entries than this are walked by a workgroup each, shorter ones by a lane group (both passes).                      */
int dgll_hip_sg_long_row(void);
/* GraphSAINT's draws.  Draw i in [0, budget) makes ONE Philox4x32-10 call with key = {seed lo, seed hi} and counter =
 * {i lo, i hi, 0, mode}; w = x0 << 32 | x1.  (Counter word 2 is 0; dgll_hip_random_walk uses its step >= 1 there: one seed may drive
 * both.)  mode 1 (node): e = mulhi64(w, nnz), the node is the row that holds entry e -- in proportion to the row lengths, with
 * replacement, rows without entries never.  mode 2 (edge): the same e, its row and col[e].  Modes 1 and 2 set the nodes' bits in
 * bitmap uint32[ceil(n_total / 32)] (cleared here), prefix int32[the same] receives the set bits below each word and info int64[8]
 * (zeroed here) = {distinct nodes, -, error bits: 2 a column id outside [0, n_total)}; they need nnz > 0.  mode 3 (walk roots):
 * roots int64[budget], roots[i] = mulhi64(w, n_total); bitmap, prefix and col are not used and may be NULL.                        */
int dgll_hip_sg_draw(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, int mode, int64_t budget,
                     uint64_t seed, uint32_t* bitmap, int32_t* prefix, int64_t* roots, int64_t* info);
/* The node set of a walk matrix (walks int32[n_entries] of dgll_hip_random_walk; -1 and ids outside [0, n_total) are skipped):
 * bitmap (cleared here), prefix and info[0] as above.                                                                            */
int dgll_hip_sg_walk_nodes(void* stream, const int32_t* walks, int64_t n_entries, int64_t n_total, uint32_t* bitmap, int32_t* prefix,
                           int64_t* info);
/* out_nodes int64[n_nodes = info[0]]: the set bits in ascending id order.                                                          */
int dgll_hip_sg_compact(void* stream, int64_t n_total, const uint32_t* bitmap, const int32_t* prefix, int64_t n_nodes, int64_t* out_nodes);


/* ---- graph embeddings: random walks and skip-gram with negative sampling (dgll_amd/embedding) -------------------------------
 * Every random word is Philox4x32-10 with key = {seed lo, seed hi}.
 * Walks: CSR (int64 rowptr, int32 col, rows ascending when p or q != 1; dgll_hip_random_walk ignores edge values)
 * over n_nodes nodes, every row shorter than 2^32; starts int64[n]; walks int32[n, length] row-major, walks[i, 0] = starts[i].
 * A node without out-edges ends the walk: every later entry is -1.  Walk i has the global index g = first_walk_index + i and step
 * s >= 1, attempt a >= 0 use the counter {g lo, g hi, s, a}: word 0 picks the candidate col[rowptr[v] + mulhi32(x0, deg)], word 1
 * accepts it when x1 < T (64-bit compare), T = round(2^32 w / M) computed here in float64 with w = 1/p when the candidate is the
 * previous node, 1 when it is an out-neighbour of the previous node, 1/q otherwise, and M = max(1/p, 1, 1/q).  The first step,
 * and every step when p == q == 1, takes attempt 0.  After max_attempts (>= 1024) rejections the last candidate is taken and
 * counted in info[0]; info[1] collects error bits (1: a start outside [0, n_nodes), 2: a column id outside it; that walk ends).
 * info: int64[2], zeroed by the caller.                                                                                       */
int dgll_hip_random_walk(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_nodes, const int64_t* starts, int64_t n,
                         int length, uint64_t first_walk_index, uint64_t seed, double p, double q, int max_attempts, int32_t* walks,
                         int64_t* info);
/* The three thresholds of dgll_hip_random_walk, {return, common neighbour, far} (host; for tests and restatements).            */
int dgll_host_node2vec_thresholds(double p, double q, uint64_t* out3);
/* Per-row alias tables for edge-weighted walks: table uint32[nnz, 2] (8-byte aligned), entry e of a row that starts at b and has
 * deg entries = {T, alias}: a draw is slot = mulhi32(x0, deg), edge = b + (x1 < T[b + slot] ? slot : alias[b + slot]), alias local
 * to the row (< deg).  Vose's construction, one lane per row, in float64 (q = val deg / sum(val), T = round(2^32 q) clamped to
 * 2^32 - 1) and in a fixed order: two builds give the same bits.  A slot that always keeps itself is {2^32 - 1, slot}.  val: fp32
 * [nnz], finite and >= 0; an edge of weight 0 is never drawn.  A row whose weights sum to 0 holds {0, slot} in every slot (no other
 * row holds such an entry) and is a dead end for the walks.  A negative, NaN or infinite weight sets bit 4 of info[1] (int64[2],
 * zeroed by the caller; info[0] is not written) and leaves its row a dead end.  scratch: 12 bytes per edge, 8-byte aligned.    */
int dgll_hip_alias_build(void* stream, const int64_t* rowptr, const float* val, int64_t n_rows, int64_t nnz, void* scratch,
                         size_t scratch_bytes, uint32_t* table, int64_t* info);
/* dgll_hip_random_walk with the candidate of every attempt drawn from `table` (dgll_hip_alias_build of this CSR's values): same
 * counters, word 0 picks the slot, word 1 keeps it or takes its alias, word 2 is the acceptance word against T (used when p or
 * q != 1 and s > 1), so P(x | t, v) is proportional to val(v, x) * w(t, x).  The first step is weighted as well.  Cap, capped
 * count, dead ends and error bits as above; bit 8 of info[1]: an alias index outside its row (the table is not this graph's).  */
int dgll_hip_random_walk_weighted(void* stream, const int64_t* rowptr, const int32_t* col, const uint32_t* table, int64_t n_nodes,
                                  const int64_t* starts, int64_t n, int length, uint64_t first_walk_index, uint64_t seed, double p,
                                  double q, int max_attempts, int32_t* walks, int64_t* info);
/* struc2vec, structural distances: exact dynamic time warping between ordered degree sequences, one task per (pair, level).
 * Sequences are ragged: the sequence of node v at BFS level l is entries [seq_ptr[v * n_levels + l], seq_ptr[v * n_levels + l + 1])
 * of seq_deg / seq_cnt (int32: a degree and how many nodes of the ring have it, degrees ascending; counts >= 1), seq_ptr
 * int64[n_nodes * n_levels + 1].  pairs: int32[n_pairs, 2] node ids in [0, n_nodes).  dist: fp64[n_pairs, n_levels] row-major,
 * D[i][j] = c + min(D[i-1][j], D[i][j-1], D[i-1][j-1]), c = ((max(da, db) + 0.5) / (min(da, db) + 0.5) - 1) * max(ca, cb), in IEEE
 * float64 without contraction; d(a, b) and d(b, a) are the same bits.  -1 from the first level at which either node's sequence is
 * empty.  The shorter sequence of a task may hold at most dgll_hip_struc_dtw_max_rows() entries (a task over it is written as NaN;
 * callers check beforehand).                                                                                                    */
int dgll_hip_struc_dtw(void* stream, const int64_t* seq_ptr, const int32_t* seq_deg, const int32_t* seq_cnt, int64_t n_nodes,
                       int n_levels, const int32_t* pairs, int64_t n_pairs, double* dist);
int dgll_hip_struc_dtw_max_rows(void);
/* struc2vec, the walk over the multilayer context graph: a stacked CSR of n_layers * n_nodes rows, row l * n_nodes + v = the
 * neighbours of v in layer l (int64 rowptr[n_layers * n_nodes + 1], int32 col holding node ids in [0, n_nodes)), `table` its
 * dgll_hip_alias_build table, t_up uint32[n_layers * n_nodes] the up-move thresholds round(2^32 x / (x + 1)), x = log(gamma + e).
 * A walk holds (v, layer), layer 0 at its start.  Step s >= 1 runs attempts a = 0, 1, ... with the counter {g lo, g hi, s, a}:
 * x0 < T_stay = round(2^32 stay_prob): stay -- slot = mulhi32(x1, deg), edge = x2 < T[slot] ? slot : alias[slot], the column is
 * emitted and the step ends; an empty or dead row ends the walk (-1 from there on).  Otherwise x3 < t_up[row]: up one layer when
 * layer + 1 < n_layers and row (layer + 1) * n_nodes + v has entries; else down one layer when layer > 0.  Attempt
 * max_attempts - 1 (max_attempts >= 1) stays whatever x0 says; every time it is reached info[0] is incremented.  walks
 * int32[n, length]; layers_out: NULL or int32[n, length], the layer every entry was emitted from (0 for the start, -1 where the
 * walk is -1).  info and its error bits as for dgll_hip_random_walk_weighted.                                                   */
int dgll_hip_struc_walk(void* stream, const int64_t* rowptr, const int32_t* col, const uint32_t* table, const uint32_t* t_up,
                        int64_t n_nodes, int n_layers, const int64_t* starts, int64_t n, int length, uint64_t first_walk_index,
                        uint64_t seed, double stay_prob, int max_attempts, int32_t* walks, int32_t* layers_out, int64_t* info);
/* Pairs of a batch of walks: centre = position j of walk w, context slot s in [0, 2 window) = position j + o, o = -window..-1,
 * 1..window; the pair exists when both positions lie in the walk and hold ids in [0, n_nodes).  Negative k of a pair is
 * searchsorted(cdf, x0, side = right) with cdf uint64[n_nodes] the noise distribution's cumulative sums scaled to 2^32
 * (cdf[n_nodes - 1] = 2^32) and x0 word 0 of the counter {g lo, g hi, j * 2 window + s, k | 2^31}.
 * out: int32[n, length, 2 window, negatives], -1 where there is no pair.                                                       */
int dgll_hip_sgns_negatives(void* stream, const int32_t* walks, int64_t n, int length, int window, int negatives,
                            const uint64_t* cdf, int64_t n_nodes, uint64_t first_walk_index, uint64_t seed, int32_t* out);
/* One batch-synchronous SGD step on sum_pairs [-log sigma(u_c . v_t) - sum_k log sigma(-u_c . v_nk)], u = rows of w_in, v = rows of
 * w_out (both fp32 [n_nodes, dim] row-major, updated in place by fp32 atomics), every gradient at the weights as the step found
 * them; a negative equal to its pair's context has coefficient 0.  *loss (fp64, device) receives the loss sum.  Scratch:
 * g_scratch fp32 and target_scratch int32 [n * length * 2 window * (1 + negatives)], delta_scratch fp32 [n * length * dim].
 * dim in [1, 4032].                                                                                                            */
int dgll_hip_sgns_step(void* stream, float* w_in, float* w_out, int64_t n_nodes, int dim, const int32_t* walks, int64_t n, int length,
                       int window, int negatives, const uint64_t* cdf, uint64_t first_walk_index, uint64_t seed, float lr,
                       float* g_scratch, int32_t* target_scratch, float* delta_scratch, double* loss);
/* Size-capped Louvain, one synchronous local-moving sweep of one level (dgll_amd/community.py runs the levels).  CSR rowptr int64
 * [n + 1], col int32 [nnz]; w: int64 [nnz] entry weights, NULL = 1 per stored entry; k int64 [n] weighted degree (self-loop entries
 * included); size int64 [n] original nodes per node; comm int32 [n] in [0, n); tot / csize int64 [n] and cnt int32 [n]: per
 * community the sum of k, of size and the member count, as they are at the start of the sweep; two_m = sum(k), in [1, 2^53).
 * Node v of community a is active when all_active != 0 or bit 0 of word 0 of Philox4x32-10 with key {seed lo, seed hi} and counter
 * {v, level, sweep, 0} is set.  With W(v, x) the summed weight of v's entries (v, u), u != v, comm[u] == x:
 *     gain(c) = (double)W(v, c) - resolution * (double)k_v * (double)tot_c / (double)two_m
 *     stay    = (double)W(v, a) - resolution * (double)k_v * (double)(tot_a - k_v) / (double)two_m
 * evaluated left to right in IEEE float64 without contraction.  target[v] = the community c != a among v's neighbours with
 * csize_c + size_v <= cap, gain(c) > stay and not (cnt_a == 1 && cnt_c == 1 && c > a) that has the largest gain, ties to the
 * smallest id; a for an inactive node or when there is none.  W is summed with integer atomics in hash tables of
 * 2 * next_pow2(deg) slots: in a wavefront's LDS for rows of up to wave_max_deg entries (<= 128, -1 = 128), in a workgroup's LDS up
 * to block_max_deg (<= 2048, -1 = 2048), in `scratch` beyond; the three give the same targets.
 * scratch: 8-byte aligned, dgll_hip_louvain_scratch_bytes(n, long_slots) bytes = 64 + 4 n + 12 long_slots (the 4-byte part padded
 * to 8), long_slots >= the sum of 2 * next_pow2(deg) over the active rows longer than block_max_deg; cleared here.
 * info: int64[2], zeroed by the caller: info[0] += nodes whose target differs from their community; info[1] |= error bits (1: a
 * column id outside [0, n), the entry is skipped; 2: scratch too small, the row keeps its community; 4: a row with 2^30 or more
 * entries or row pointers outside [0, nnz]; 8: a community id outside [0, n)).                                                  */
int dgll_hip_louvain_move(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* w, const int64_t* k,
                          const int64_t* size, const int32_t* comm, const int64_t* tot, const int64_t* csize, const int32_t* cnt,
                          int64_t n, int64_t nnz, int64_t two_m, double resolution, int64_t cap, uint64_t seed, uint32_t level,
                          uint32_t sweep, int all_active, int wave_max_deg, int block_max_deg, void* scratch, size_t scratch_bytes,
                          int32_t* target, int64_t* info);
size_t dgll_hip_louvain_scratch_bytes(int64_t n, int64_t long_slots);
/* Leiden's refinement, one synchronous sweep of one level (dgll_amd/community.py runs the sweeps and the levels).  The level's
 * graph, k, size, two_m, cap, the tiers, `scratch` (same layout and size rule, over all rows longer than block_max_deg) and `info`
 * as for dgll_hip_louvain_move.  bound int32 [n] in [0, n): the community local moving found, which a node never leaves here; totP
 * int64 [n]: the sum of k per bound community; sub int32 [n] in [0, n): the sub-communities at the start of the sweep, tot / csize /
 * cnt theirs.  Only the entries (v, u) with u != v and bound[u] == bound[v] count; W(v, S) is their weight into sub-community S.
 * First pass, every row: wC[v] = sum over S of W(v, S), wS[v] = W(v, sub[v]), cut[S] = sum over the members of S of wC - wS (the
 * weight between S and the rest of its bound community; integer atomics, zeroed here).  Second pass: node v of bound community p
 * decides when cnt[sub[v]] == 1 and (double)wC[v] >= resolution * (double)k_v * (double)(totP_p - k_v) / (double)two_m; then
 * target[v] = the sub-community S != sub[v] among v's neighbours in p with csize_S + size_v <= cap, not (cnt_S == 1 && S > sub[v]),
 *     (double)cut_S >= resolution * (double)tot_S * (double)(totP_p - tot_S) / (double)two_m     and
 *     gain(S) = (double)W(v, S) - resolution * (double)k_v * (double)tot_S / (double)two_m > 0
 * that has the largest gain, ties to the smallest id; sub[v] for every other node.  Float64 left to right, no contraction.
 * info[0] += nodes whose target differs from their sub-community; info[1] |= the error bits of dgll_hip_louvain_move (8: a
 * sub-community id outside [0, n)) and 16: a bound id outside [0, n) (the node keeps its sub-community, its sums are 0).        */
int dgll_hip_leiden_refine(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* w, const int64_t* k,
                           const int64_t* size, const int32_t* sub, const int32_t* bound, const int64_t* tot, const int64_t* csize,
                           const int32_t* cnt, const int64_t* totP, int64_t n, int64_t nnz, int64_t two_m, double resolution,
                           int64_t cap, int wave_max_deg, int block_max_deg, void* scratch, size_t scratch_bytes, int32_t* target,
                           int64_t* wS, int64_t* wC, int64_t* cut, int64_t* info);


/* ---- a10: H = relu(A_csr . (X[:, :actual_F] . W[:actual_F, :])) --------------------------------------------
 * launch_gcn_fused_kernel is the reference's own symbol with its exact signature
 * (/root/reference/dgll/FusedKernel/gcn_fused_kernel.cu:190-195, bound at gcn_extension.cpp:5-10,46-55): int32 CSR,
 * fp32, default stream, synchronous, `num_neighbors` = diff(row_ptr); a libgcn replacement can be relinked against
 * this library unchanged.  dgll_hip_gcn_fused_forward is the same computation with this library's conventions
 * (explicit stream, caller-owned workspace of dgll_hip_gcn_fused_workspace_bytes(), error code).               */
void launch_gcn_fused_kernel(const int* row_ptr, const int* col_idx, const float* values, const float* X, const float* W,
                             float* H, const int* num_neighbors, int N, int F_padded, int actual_F, int H_dim,
                             int total_nnz);
/* The backward twin with the reference's exact signature (gcn_fused_kernel.cu:238-244).  Computes the gradient of the
 * forward above -- G = grad_output * (A.X.W > 0), grad_W[:actual_F] = (A.X)^T.G, grad_X[:, :actual_F] = A^T.(G.W^T) --
 * not the reference kernel's known-wrong arithmetic.  Default stream, synchronous.        */
void launch_gcn_fused_kernel_backward_optimized(const int* row_ptr, const int* col_idx, const float* values,
                                                const float* X, const float* W, const float* grad_output,
                                                float* grad_W, float* grad_X, const int* num_neighbors,
                                                int N, int F_padded, int actual_F, int H_dim, int total_nnz);
int dgll_hip_gcn_fused_forward(void* stream, const int32_t* row_ptr, const int32_t* col_idx, const float* values,
                               const float* X, const float* W, float* H, int N, int F_padded, int actual_F, int H_dim,
                               int total_nnz, void* workspace, size_t workspace_bytes);
size_t dgll_hip_gcn_fused_workspace_bytes(int N, int actual_F, int H_dim);

/* ---- GATv2 (dynamic attention): the three gather passes of one layer behind one entry point (csrc/gatv2.hip) --------------------
 * Per head of width D, over the rows i of a CSR matrix A [n_dst x n_src] (rectangular allowed; edge values are not read, duplicate
 * entries are separate edges):
 *     z_ij = xl[j] + xr[i]     e_ij = attn . lrelu(z_ij, slope)     alpha = softmax over row i     out[i] = sum_j alpha_ij xl[j]
 * an empty row gives out[i] = 0.  Nothing is stored per edge; the backward passes recompute alpha_ij from lse.
 *   DGLL_GATV2_FORWARD     rowptr / col = A, n_rows = n_dst, n_cols = n_src.  Reads xl, xr, attn; writes out [n_dst, heads * D] of
 *                          `dtype` and lse fp32 [n_dst, heads] (log-sum-exp of the row's logits; 0 for an empty row).
 *   DGLL_GATV2_ROWS        the same A.  Reads xl, xr, attn, grad_out [n_dst, heads * D], lse; writes out = grad_xr [n_dst, heads * D],
 *                          lse_delta fp32 [n_dst, 2 * heads] ({lse_i | delta_i} side by side per row, delta_i = <grad_out_i, out_i>
 *                          formed in fp32) and dattn_part fp32 [dattn_blocks, heads * D]: one partial of grad_attn per workgroup, EVERY
 *                          row of it written -- and, when dattn is non-NULL, dattn fp32 [heads * D] = their sum over the first
 *                          dimension in workgroup order (a second small kernel).
 *   DGLL_GATV2_TRANSPOSED  rowptr / col = A^T, n_rows = n_src, n_cols = n_dst.  Reads xl, xr, attn, grad_out, lse_delta; writes
 *                          out = grad_xl [n_src, heads * D] (zeros for a source no row references).
 * Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned
 * bases; D a multiple of the vector width (4 fp32 / 8 bf16 columns), at most 64 vectors.  attn fp32 [heads * D].  Rows longer than
 * DGLL_GATV2_LONG_ROW entries are swept by a whole workgroup.  No float atomics: two runs give the same bits.  No pass allocates,
 * synchronises or reads anything back: the calls can be captured into a graph.                                                    */
enum { DGLL_GATV2_FORWARD = 0, DGLL_GATV2_ROWS = 1, DGLL_GATV2_TRANSPOSED = 2 };
#define DGLL_GATV2_LONG_ROW 256
typedef struct dgll_gatv2_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; int64_t n_rows; int64_t n_cols;
    int heads; int D; float slope;
    const void* xl; int64_t ld_xl;
    const void* xr; int64_t ld_xr;
    const float* attn;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    float* lse;
    float* lse_delta;
    float* dattn_part; int64_t dattn_blocks; float* dattn;
} dgll_gatv2_desc;
int dgll_hip_gatv2_pass(void* stream, const dgll_gatv2_desc* d);

/* ---- Sparse scaled dot-product attention: the three gather passes of one layer behind one entry point (csrc/sparse_attn.hip) ------
 * Per head of width D, over the rows i of a CSR matrix A [n_dst x n_src] (rectangular allowed; edge values are not read, duplicate
 * entries are separate edges):
 *     s_ij = scale <q[i], k[j]>     alpha = softmax over row i     out[i] = sum_j alpha_ij v[j]     lse[i] = log sum_j exp s_ij
 * an empty row gives out[i] = 0 and lse[i] = 0.  `scale` is an argument and is never derived from D (the layers pad D).  Nothing is
 * stored per edge; the backward passes recompute alpha_ij from lse.  With g = grad_out:
 *   DGLL_ATTN_FORWARD  rowptr / col = A, n_rows = n_dst, n_cols = n_src.  Reads q, k, v; writes out [n_dst, heads * D] of `dtype` and
 *                      lse fp32 [n_dst, heads].
 *   DGLL_ATTN_ROWS     the same A.  Reads q, k, v, grad_out [n_dst, heads * D], lse; writes out = grad_q [n_dst, heads * D] and
 *                      lse_delta fp32 [n_dst, 2 * heads] ({lse_i | delta_i} side by side per row, delta_i = sum_j alpha_ij <g_i, v_j>
 *                      formed in fp32).
 *   DGLL_ATTN_COLS     rowptr / col = A^T, n_rows = n_src, n_cols = n_dst.  Reads q, k, v, grad_out, lse_delta; writes out = grad_k and
 *                      out2 = grad_v, both [n_src, heads * D] (zeros for a source no row references).
 * kv_shared != 0: k and v are the same buffer (same pointer and pitch); the forward and the rows pass load each source row once.
 * The cols pass still writes grad_k and grad_v separately.
 * Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned
 * bases; D a multiple of the vector width (4 fp32 / 8 bf16 columns), at most 64 vectors.  Rows longer than DGLL_ATTN_LONG_ROW
 * entries are swept by a whole workgroup.  No float atomics: two runs give the same bits.  No pass allocates, synchronises or reads
 * anything back: the calls can be captured into a graph.                                                                          */
enum { DGLL_ATTN_FORWARD = 0, DGLL_ATTN_ROWS = 1, DGLL_ATTN_COLS = 2 };
#define DGLL_ATTN_LONG_ROW 256
typedef struct dgll_attn_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; int64_t n_rows; int64_t n_cols;
    int heads; int D; float scale; int kv_shared;
    const void* q; int64_t ld_q;
    const void* k; int64_t ld_k;
    const void* v; int64_t ld_v;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    void* out2; int64_t ld_out2;
    float* lse;
    float* lse_delta;
} dgll_attn_desc;
int dgll_hip_sparse_attn_pass(void* stream, const dgll_attn_desc* d);

/* ---- Typed-edge basis aggregation (R-GCN / RelGraphConv): three gather passes behind one entry point (csrc/typed_spmm.hip) --------
 * Every entry e of a CSR matrix A [n_dst x n_src] (rectangular allowed, duplicate entries are separate edges) carries a type
 * etype[e] in [0, R) and optionally a factor norm[e] (NULL: 1).  With the coefficient table coeff fp32 [R, B] (row-major):
 *     Z[i, b, :] = sum_{e = (j -> i)} norm[e] * coeff[etype[e], b] * X[j, :]          Z: [n_dst, B * F], basis-major blocks of width F
 *   DGLL_TYPED_EXPAND     rowptr / col / etype / norm = A, n_rows = n_dst, n_cols = n_src.  Reads x [n_src, F]; writes out = Z
 *                         [n_dst, B * F] of `dtype` (zeros for an empty row).
 *   DGLL_TYPED_CONTRACT   rowptr / col = A^T with etype / norm in A^T's entry order, n_rows = n_src, n_cols = n_dst.  Reads dz
 *                         [n_dst, B * F]; writes out = dX [n_src, F], dX[j] = sum_e norm[e] sum_b coeff[etype[e], b] dz[i_e, b, :]
 *                         (zeros for a source no row references).
 *   DGLL_TYPED_EDGE_DOTS  rowptr / col = A.  Reads x [n_src, F] and dz [n_dst, B * F]; writes p fp32 [nnz, ld_p], ld_p = B rounded
 *                         up to 4: p[e, b] = <x[j_e], dz[i_e, b, :]>, the padding columns zeros.  etype, norm and coeff are not read
 *                         (norm is NOT applied): grad coeff[r, b] = sum over the entries of type r of norm[e] p[e, b].
 * Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned
 * bases; F a multiple of the vector width (4 fp32 / 8 bf16 columns).  Any B >= 1: bases are taken DGLL_TYPED_BASIS_BLOCK at a time,
 * more of them re-gather x once per block.  coeff goes through LDS when R * B <= DGLL_TYPED_COEFF_LDS entries, else it is read from
 * global memory.  The type used for addressing is clamped to [0, R): the caller validates the range (dgll_amd/ops_typed.py does,
 * once per edge set).  Rows longer than DGLL_TYPED_LONG_ROW entries are swept by a whole workgroup.  No atomics: two runs give the
 * same bits.  No pass allocates, synchronises or reads anything back: the calls can be captured into a graph.                      */
enum { DGLL_TYPED_EXPAND = 0, DGLL_TYPED_CONTRACT = 1, DGLL_TYPED_EDGE_DOTS = 2 };
#define DGLL_TYPED_LONG_ROW 256
#define DGLL_TYPED_COEFF_LDS 4096
#define DGLL_TYPED_BASIS_BLOCK 8
typedef struct dgll_typed_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; const int32_t* etype; const float* norm;
    int64_t n_rows; int64_t n_cols;
    int R; int B; int64_t F;
    const float* coeff;
    const void* x; int64_t ld_x;
    const void* dz; int64_t ld_dz;
    void* out; int64_t ld_out;
    float* p; int64_t ld_p;
} dgll_typed_desc;
int dgll_hip_typed_spmm_pass(void* stream, const dgll_typed_desc* d);

/* ---- Per-edge message passing (DGL's edge_softmax, u_mul_e_sum, u_dot_v, u_add_v, copy_e_sum): six passes behind one entry point
 * (csrc/mp_ops.hip).  The general path under the fused layers: per-edge tensors EXIST here, fp32 [nnz, heads] each.
 * Entry k of the pass's CSR (rowptr / col: n_rows rows gathering from n_cols; rectangular allowed, duplicate entries are separate
 * edges) belongs to row i(k) and addresses the per-edge arrays at slot s(k) = perm ? perm[k] : k.  With perm (A^T's entry -> A's
 * entry, graph.transpose()) a pass runs over A^T while the per-edge data stays in A's entry order; `nnz` is the number of rows of
 * the per-edge arrays.  perm and col values used for addressing are clamped to [0, nnz) and [0, n_cols).  Per head h:
 *   DGLL_MP_EDGE_SOFTMAX      e_out[s(k), h] = exp(e[s(k), h] - m_ih) / l_ih over the entries of row i (max-subtracted).  An entry
 *                             of -inf gives 0; a row of -inf alone, like an empty row, writes zeros and never NaN.
 *   DGLL_MP_EDGE_SOFTMAX_BWD  e = alpha (the forward's output), e2 = grad: e_out[s, h] = alpha (g - sum_row alpha g), the row sum in fp32.
 *   DGLL_MP_E_SUM             out[i, h] = sum_k e[s(k), h]; out fp32 [n_rows, heads] (an empty row: 0); dtype must be DGLL_F32.
 *   DGLL_MP_U_ADD_V           e_out[s(k), h] = x[col_k, h] + y[i(k), h]; x [n_cols, heads] and y [n_rows, heads] fp32, either may be
 *                             NULL (0; col is read only with x); dtype must be DGLL_F32.
 *   DGLL_MP_U_MUL_E_SUM       out[i, h*D : (h+1)*D] = sum_k e[s(k), h] * x[col_k, h*D : (h+1)*D]; x and out of `dtype` (an empty row: 0).
 *   DGLL_MP_U_DOT_V           e_out[s(k), h] = <x[col_k, h, :], y[i(k), h, :]>; x and y of `dtype`, products and sum in fp32.
 * Per-edge arrays are always fp32 with pitches ld_e* >= heads, any heads >= 1 (D is not read by the first four passes).  The node
 * matrices of the last two are of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches in elements: whole 16-byte vectors,
 * 16-byte aligned bases; D a multiple of the vector width (4 fp32 / 8 bf16 columns), at most 64 vectors.  Rows longer than
 * DGLL_MP_LONG_ROW entries are swept by a whole workgroup.  No float atomics: two runs give the same bits.  No pass allocates,
 * synchronises or reads anything back: the calls can be captured into a graph.  n_rows == 0 launches nothing.                     */
enum { DGLL_MP_EDGE_SOFTMAX = 0, DGLL_MP_EDGE_SOFTMAX_BWD = 1, DGLL_MP_E_SUM = 2,
       DGLL_MP_U_ADD_V = 3, DGLL_MP_U_MUL_E_SUM = 4, DGLL_MP_U_DOT_V = 5 };
#define DGLL_MP_LONG_ROW 256
typedef struct dgll_mp_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int heads; int D;
    const float* e;  int64_t ld_e;
    const float* e2; int64_t ld_e2;
    float* e_out;    int64_t ld_e_out;
    const void* x; int64_t ld_x;
    const void* y; int64_t ld_y;
    void* out; int64_t ld_out;
} dgll_mp_desc;
int dgll_hip_mp_pass(void* stream, const dgll_mp_desc* d);

/* ---- Multi-aggregator gather (PNA / DGL's PNAConv): several reductions of a neighbourhood from ONE gather, three passes behind one
 * entry point (csrc/multi_agg.hip).  rowptr / col: a CSR matrix [n_rows x n_cols] (rectangular allowed; edge values are not read;
 * duplicate entries are separate edges).  The descriptor carries the ORDERED lists the caller asked for: n_agg <= 6 aggregator codes
 * agg[] and n_scaler <= 3 scaler codes scaler[], no repeats.  Over the D_i entries j of row i, x the gathered matrix [n_cols, F] and y
 * an optional per-row addend [n_rows, F] (NULL: 0):
 *     DGLL_MAGG_MEAN  mean_j x[j] + y[i]           DGLL_MAGG_SUM  sum_j x[j] + D_i y[i]
 *     DGLL_MAGG_MAX   max_j x[j] + y[i]            DGLL_MAGG_MIN  min_j x[j] + y[i]
 *     DGLL_MAGG_VAR   relu(mean_j x[j]^2 - (mean_j x[j])^2)   (y does not enter)        DGLL_MAGG_STD  sqrt(VAR + 1e-30)
 * and the per-row scalers, delta > 0:  DGLL_MAGG_IDENTITY 1, DGLL_MAGG_AMPLIFICATION log(D_i + 1) / delta, DGLL_MAGG_ATTENUATION
 * delta / log(D_i + 1).  A row WITHOUT entries writes zeros in every block (y and the scalers do not apply).  The variance is
 * accumulated about the row's first entry: a row whose entries are all equal gives exactly VAR = 0 and STD = sqrt(1e-30).
 *   DGLL_MAGG_FORWARD  rowptr / col = A.  Reads x and optionally y; writes out [n_rows, n_scaler * n_agg * F] of `dtype`, block
 *                      (s * n_agg + a) = scaler_s(i) * agg_a(i) (DGL's concatenation order); optionally stats fp32 [n_rows, 2 F]:
 *                      mean | variance of x over the row (without y), and arg int32 [n_rows, 2 F]: the source row attaining the
 *                      max | min per column, -1 for an empty row.  TIES: among the entries attaining the extreme, the smallest
 *                      source id (torch gives the gradient to an unspecified one of them: the results differ on ties only).
 *   DGLL_MAGG_ROWS     no gather.  Reads grad_out (the shape of out), rowptr and stats (required with coef when VAR or STD is
 *                      asked); folds the scalers and writes coef fp32 [n_rows, 5 F] = c0 | c1 | mean | g_max | g_min with
 *                      c0 = g_sum + g_mean / D_i and c1 = (2 g_var + g_std / std_i) / D_i where var_i > 0, EXACTLY 0 elsewhere; and
 *                      grad_y [n_rows, F] of `dtype` = g_mean + g_max + g_min + D_i g_sum (0 for an empty row).  Either output may be
 *                      NULL, not both.
 *   DGLL_MAGG_COLS     rowptr / col = A^T with sorted rows (n_rows = A's n_cols).  Reads x [n_rows, F] (held), coef and arg of A's
 *                      rows; writes grad_x [n_rows, F] of `dtype` (zeros for a source no row references):
 *                          grad_x[j] = sum_{i in row j} c0_i + c1_i (x[j] - mean_i) + (argmax_i == j) g_max_i + (argmin_i == j) g_min_i
 *                      the variance term formed per entry; a repeated (j, i) pair counts once for max / min, as in
 *                      dgll_hip_segment_max_bwd.  arg is required when MAX or MIN is asked.
 * Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned
 * bases; stats, arg and coef likewise (pitches multiples of 4).  F a positive multiple of the vector width (4 fp32 / 8 bf16 columns);
 * widths past 64 vectors go to column blocks.  Indices used for addressing are clamped.  Rows longer than DGLL_MAGG_LONG_ROW entries
 * are swept by a whole workgroup and merged through LDS in group order.  No atomics: two runs give the same bits.  No pass allocates,
 * synchronises or reads anything back: the calls can be captured into a graph.  n_rows == 0 launches nothing.                       */
enum { DGLL_MAGG_FORWARD = 0, DGLL_MAGG_ROWS = 1, DGLL_MAGG_COLS = 2 };
enum { DGLL_MAGG_MEAN = 0, DGLL_MAGG_SUM = 1, DGLL_MAGG_MAX = 2, DGLL_MAGG_MIN = 3, DGLL_MAGG_VAR = 4, DGLL_MAGG_STD = 5 };
enum { DGLL_MAGG_IDENTITY = 0, DGLL_MAGG_AMPLIFICATION = 1, DGLL_MAGG_ATTENUATION = 2 };
#define DGLL_MAGG_LONG_ROW 256
typedef struct dgll_multi_agg_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; int64_t n_rows; int64_t n_cols;
    int64_t F;
    int n_agg; int agg[6]; int n_scaler; int scaler[3]; float delta;
    const void* x; int64_t ld_x;
    const void* y; int64_t ld_y;
    void* out; int64_t ld_out;
    const void* grad_out; int64_t ld_grad_out;
    float* stats; int64_t ld_stats;
    int32_t* arg; int64_t ld_arg;
    float* coef; int64_t ld_coef;
    void* grad_y; int64_t ld_grad_y;
    void* grad_x; int64_t ld_grad_x;
} dgll_multi_agg_desc;
int dgll_hip_multi_agg_pass(void* stream, const dgll_multi_agg_desc* d);

/* ---- Edge-feature aggregation (DGL's GINEConv, CFConv): a gather-reduce whose message combines the gathered source row with a
 * per-edge row of the SAME width, and its exact backward; three passes behind one entry point (csrc/edge_feat.hip).  Entry k of row
 * i of A (rowptr / col, [n_dst x n_src], rectangular allowed, edge values are not read) is the edge j = col[k] -> i and e[k, :] its
 * feature row, in A's entry order; duplicate entries are separate edges with their own rows.  scale: an optional fp32 factor s_i per
 * DESTINATION row (NULL: 1; the mean reduce passes 1 / D_i, 0 for an empty row).  op chooses the message:
 *     DGLL_EF_ADD       m = x_j + e_k          dm/dx = 1        dm/de = 1
 *     DGLL_EF_ADD_RELU  m = relu(x_j + e_k)    dm/dx = gate_k   dm/de = gate_k      gate_k = (x_j + e_k > 0)
 *     DGLL_EF_MUL       m = x_j * e_k          dm/dx = e_k      dm/de = x_j
 * The gate is recomputed from the stored operands as the same fp32 sum in every pass and never stored.
 *   DGLL_EF_FORWARD  rowptr / col = A (n_rows = n_dst, n_cols = n_src).  out[i] = s_i * sum_k m(x[col_k], e[k]); reads x [n_cols, F]
 *                    (gathered), e [nnz, F] (streamed at slot k), scale [n_rows]; writes out [n_rows, F] (an empty row: zeros).
 *   DGLL_EF_COLS     rowptr / col = A^T (n_rows = n_src, n_cols = n_dst) with perm, A^T's entry k' -> A's entry (graph.transpose()).
 *                    grad_x[j] = sum_k' s_i dm/dx grad_out[i], i = col[k']; reads grad_out [n_cols, F] (gathered), scale [n_cols]
 *                    (by the gathered row), x [n_rows, F] (held; ADD_RELU only), e at slot perm[k'] (ADD_RELU and MUL; perm is then
 *                    required); writes grad_x [n_rows, F] (zeros for a source no row references).
 *   DGLL_EF_EDGE     rowptr / col = A.  grad_e[k] = s_i dm/de grad_out[i]; reads grad_out [n_rows, F] (held), x gathered (ADD_RELU
 *                    and MUL), e at slot k (ADD_RELU); writes grad_e [nnz, F] of `dtype`.  No reduction.
 * Operands a (pass, op) does not read may be NULL and are not dereferenced.  nnz: the rows of e / grad_e (perm values are clamped
 * to [0, nnz), col values used for addressing to [0, n_cols)).  Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation),
 * pitches ld_* in elements, each its own: whole 16-byte vectors >= F, 16-byte aligned bases.  F a positive multiple of the vector
 * width (4 fp32 / 8 bf16 columns); widths past 64 vectors go to column blocks.  Rows longer than DGLL_EF_LONG_ROW entries are swept
 * by a whole workgroup and, where there is a sum, merged through LDS in group order.  No atomics: two runs give the same bits.  No
 * pass allocates, synchronises or reads anything back: the calls can be captured into a graph.  n_rows == 0 launches nothing.       */
enum { DGLL_EF_FORWARD = 0, DGLL_EF_COLS = 1, DGLL_EF_EDGE = 2 };
enum { DGLL_EF_ADD = 0, DGLL_EF_ADD_RELU = 1, DGLL_EF_MUL = 2 };
#define DGLL_EF_LONG_ROW 256
typedef struct dgll_edge_feat_desc {
    int pass; int dtype; int op;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int64_t F;
    const float* scale;
    const void* x; int64_t ld_x;
    const void* e; int64_t ld_e;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    void* grad_x; int64_t ld_grad_x;
    void* grad_e; int64_t ld_grad_e;
} dgll_edge_feat_desc;
int dgll_hip_edge_feat_pass(void* stream, const dgll_edge_feat_desc* d);

/* ---- Edge-gated aggregation with edge outputs (Bresson & Laurent's residual gated graph convnet, DGL's GatedGCNConv) and its exact
 * backward; three passes behind one entry point (csrc/gated.hip).  Entry k of row i of A (rowptr / col, [n_dst x n_src], rectangular
 * allowed, edge values are not read) is the edge j = col[k] -> i; per-edge matrices are in A's entry order; duplicate entries are
 * separate edges.  For every column independently, with a [n_dst, F], b and v [n_src, F], c [nnz, F]:
 *     ehat[k] = c[k] + a[i] + b[j]     sig[k] = sigmoid(ehat[k])     S_i = sum_k sig[k] + eps     out[i] = (sum_k sig[k] v[j]) / S_i
 * ehat is rounded to `dtype` when stored and every pass, the forward included, takes the sigmoid of that stored value (fp32, exp2 form;
 * a saturated gate is exactly 0 or 1), so the gate itself is never stored.  With g = grad_out and ge = grad_ehat (NULL: zeros):
 *     t[k] = ge[k] + g[i] (v[j] - out[i]) / S_i sig[k] (1 - sig[k])      grad_c[k] = t[k]      grad_a[i] = sum over row i of t[k]
 *     grad_b[j] = sum over column j of t[k]                               grad_v[j] = sum over column j of sig[k] g[i] / S_i
 *   DGLL_GATED_FORWARD  rowptr / col = A (n_rows = n_dst, n_cols = n_src).  Reads a (held), b and v (gathered), c (streamed at slot k);
 *                       writes ehat [nnz, F], out [n_rows, F] (a row without entries: zeros) and the fp32 row state inv_s = 1 / S_i and
 *                       out32 = the unrounded out_i, both [n_rows, F].
 *   DGLL_GATED_ROWS     rowptr / col = A.  Reads grad_out, inv_s, out32 (held), v (gathered), ehat and grad_ehat (optional) at slot k;
 *                       writes grad_c [nnz, F] (t, rounded to `dtype`), grad_a [n_rows, F] (the fp32 sum of the unrounded t) and, when
 *                       w is non-NULL, w [n_rows, F] = grad_out / S_i for the cols pass.  grad_c and grad_a go together; with both NULL
 *                       the pass reads no per-edge operand and only leaves w.
 *   DGLL_GATED_COLS     rowptr / col = A^T (n_rows = n_src, n_cols = n_dst) with perm, A^T's entry k' -> A's entry (graph.transpose()).
 *                       grad_b [n_rows, F] (when non-NULL) sums grad_c at slot perm[k'], the stored and so rounded t; grad_v [n_rows, F]
 *                       (when non-NULL) sums sigmoid(ehat at slot perm[k']) * w[col[k']].  At least one of the two; zeros for a source
 *                       no row references.
 * Operands a pass does not read may be NULL and are not dereferenced.  nnz: the rows of the per-edge matrices (perm values are clamped
 * to [0, nnz), col values used for addressing to [0, n_cols)).  Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation) but
 * for the fp32 row state; pitches ld_* in elements, each its own: whole 16-byte vectors of `dtype` >= F, 16-byte aligned bases.  F a
 * positive multiple of the vector width (4 fp32 / 8 bf16 columns); widths past 64 vectors go to column blocks.  Rows longer than
 * DGLL_GATED_LONG_ROW entries are swept by a whole workgroup and merged through LDS in group order.  No atomics: two runs give the
 * same bits.  No pass allocates, synchronises or reads anything back: the calls can be captured into a graph.  n_rows == 0 launches
 * nothing.                                                                                                                           */
enum { DGLL_GATED_FORWARD = 0, DGLL_GATED_ROWS = 1, DGLL_GATED_COLS = 2 };
#define DGLL_GATED_LONG_ROW 256
typedef struct dgll_gated_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int64_t F; float eps;
    const void* a; int64_t ld_a;
    const void* b; int64_t ld_b;
    const void* c; int64_t ld_c;
    const void* v; int64_t ld_v;
    void* out; int64_t ld_out;
    void* ehat; int64_t ld_ehat;
    float* inv_s; int64_t ld_inv_s;
    float* out32; int64_t ld_out32;
    const void* grad_out; int64_t ld_grad_out;
    const void* grad_ehat; int64_t ld_grad_ehat;
    void* grad_c; int64_t ld_grad_c;
    void* grad_a; int64_t ld_grad_a;
    void* w; int64_t ld_w;
    void* grad_b; int64_t ld_grad_b;
    void* grad_v; int64_t ld_grad_v;
} dgll_gated_desc;
int dgll_hip_gated_pass(void* stream, const dgll_gated_desc* d);

/* ---- Gated aggregation with nothing stored per edge (the residual gated graph convnet without edge features: PyG's
 * ResGatedGraphConv) and its exact backward; three passes behind one entry point (csrc/res_gated.hip).  Entry e of row i of A
 * (rowptr / col, [n_dst x n_src], rectangular allowed, edge values are not read) is the edge j = col[e] -> i; duplicate entries are
 * separate edges.  For every column independently, with k [n_dst, F], q and v [n_src, F] and g = grad_out [n_dst, F]:
 *     s = sigmoid(k[i] + q[j])        out[i] = sum_e s v[j]        (mean != 0: divided by the row's entry count)
 *     grad_k[i] = g[i] sum_e s (1 - s) v[j]      grad_q[j] = v[j] sum over column j of g[i] s (1 - s)      grad_v[j] = sum over column j of g[i] s
 * The gate is the same fp32 function of the same stored k and q in every pass (1 / (1 + exp2(-x log2 e)): a saturated gate is exactly
 * 0 or 1, and s (1 - s) then exactly 0) and is never stored: no pass reads or writes an [nnz, F] array.
 *   DGLL_RES_GATED_FORWARD  rowptr / col = A (n_rows = n_dst, n_cols = n_src).  Reads k (held), q and v (gathered); writes out
 *                           [n_rows, F] (a row without entries: zeros), scaled by 1 / (its entry count) in fp32 before the one store
 *                           when mean != 0.
 *   DGLL_RES_GATED_ROWS     rowptr / col = A.  Reads k and grad_out (held), q and v (gathered); writes grad_k [n_rows, F].
 *   DGLL_RES_GATED_COLS     rowptr / col = A^T (n_rows = n_src, n_cols = n_dst; graph.transpose()'s structure, its permutation is not
 *                           used).  Reads q (held), k and grad_out (gathered at col[e']) and, for grad_q, v (the row's own, at its end);
 *                           writes grad_q and grad_v [n_rows, F], either of which may be NULL (not both): what only the missing one
 *                           needs is neither loaded nor summed.  Zeros for a source no row references.
 * `mean` is read by FORWARD alone (the backward of a mean takes grad_out already divided by the entry counts).  col values used for
 * addressing are clamped to [0, n_cols).  Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation); pitches ld_* in elements,
 * each its own: whole 16-byte vectors of `dtype` >= F, 16-byte aligned bases; the columns behind F are never read into a result and
 * never written.  F a positive multiple of the vector width (4 fp32 / 8 bf16 columns); widths past 64 vectors go to column blocks.
 * Rows longer than DGLL_RES_GATED_LONG_ROW entries are swept by a whole workgroup and merged through LDS in group order.  No atomics:
 * two runs give the same bits.  No pass allocates, synchronises or reads anything back: the calls can be captured into a graph.
 * n_rows == 0 launches nothing.                                                                                                      */
enum { DGLL_RES_GATED_FORWARD = 0, DGLL_RES_GATED_ROWS = 1, DGLL_RES_GATED_COLS = 2 };
#define DGLL_RES_GATED_LONG_ROW 256
typedef struct dgll_res_gated_desc {
    int pass; int dtype;
    const int64_t* rowptr; const int32_t* col; int64_t n_rows; int64_t n_cols;
    int64_t F; int mean;
    const void* k; int64_t ld_k;
    const void* q; int64_t ld_q;
    const void* v; int64_t ld_v;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    void* grad_k; int64_t ld_grad_k;
    void* grad_q; int64_t ld_grad_q;
    void* grad_v; int64_t ld_grad_v;
} dgll_res_gated_desc;
int dgll_hip_res_gated_pass(void* stream, const dgll_res_gated_desc* d);

/* ---- Edge-feature aggregation with the edge projection fused in (PyG's GINEConv(edge_dim=)): dgll_hip_edge_feat_pass's message with
 * e_k formed per entry in registers from the raw edge attributes, so that no pass reads or writes an [nnz, F] array
 * (csrc/edge_proj.hip).  Entry k of row i of A is the edge j = col[k] -> i and a[k, :] its De attributes, in A's entry order.  With
 * weight [De, F] and bias [F] (or NULL: 0), both fp32 and contiguous, and op / scale as dgll_hip_edge_feat_pass (DGLL_EF_ADD,
 * DGLL_EF_ADD_RELU, DGLL_EF_MUL):
 *     e_k = bias + sum_d a[k, d] weight[d, :]       fp32, from bias, d ascending, one fused multiply-add per term: the same bits in
 *                                                   every pass, so the relu of the forward and the gates of the backward agree
 *     t_k = s_i dm/de grad_out[i]                   (never stored)
 *   DGLL_EFP_FORWARD  rowptr / col = A.  out[i] = s_i sum_k m(x[col_k], e_k); reads x (gathered), a at slot k; writes out [n_rows, F].
 *   DGLL_EFP_COLS     rowptr / col = A^T with perm (graph.transpose()).  grad_x[j] = sum_k' s_i dm/dx grad_out[i]; reads grad_out
 *                     (gathered), scale (by the gathered row), x (held; ADD_RELU), a at slot perm[k']; writes grad_x [n_rows, F].
 *                     ADD_RELU and MUL only: the grad_x of ADD reads neither x nor e and is dgll_hip_edge_feat_pass's DGLL_EF_COLS.
 *   DGLL_EFP_PARAM    rowptr / col = A.  `partials` workgroups take the row tiles grid-stride; each writes one slab
 *                     slabs[p] = [De + 1, F] fp32: rows d < De the workgroup's share of grad_weight[d] = sum_k a[k, d] t_k, row De
 *                     that of grad_bias = sum_k t_k.  The caller sums the slabs in slab order.  Reads grad_out (held), a, x
 *                     (gathered; ADD_RELU, MUL), weight and bias (ADD_RELU).  Every element of every slab is written.
 *   DGLL_EFP_DOTS     rowptr / col = A.  grad_a[k, d] = sum over the columns of weight[d, :] t_k, in `dtype`; reads grad_out (held),
 *                     weight, x (gathered; ADD_RELU, MUL), a and bias (ADD_RELU).  Past one column block (F > 64 lane vectors) the
 *                     per-block partial dots go to dots_part [col_blocks, nnz, De] fp32 instead (required then; the caller sums them in
 *                     block order) and grad_a is not written.  Columns of grad_a's pitch past De are not written.
 * 1 <= De <= DGLL_EFP_MAX_DE.  a: `dtype`, pitch ld_a of whole 16-byte vectors >= De; the columns past De are never read into a
 * result.  Operands a (pass, op) does not read may be NULL and are not dereferenced.  Everything else (dtype, pitches, F, column
 * blocks, long rows, clamped col / perm, no atomics, nothing allocated, synchronised or read back, n_rows == 0) as
 * dgll_hip_edge_feat_pass.                                                                                                          */
enum { DGLL_EFP_FORWARD = 0, DGLL_EFP_COLS = 1, DGLL_EFP_PARAM = 2, DGLL_EFP_DOTS = 3 };
#define DGLL_EFP_LONG_ROW 256
#define DGLL_EFP_MAX_DE 16
#define DGLL_EFP_MAX_PARTIALS 512
typedef struct dgll_edge_proj_desc {
    int pass; int dtype; int op; int De;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int64_t F;
    const float* scale;
    const void* x; int64_t ld_x;
    const void* a; int64_t ld_a;
    const float* weight; const float* bias;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    void* grad_x; int64_t ld_grad_x;
    void* grad_a; int64_t ld_grad_a;
    float* dots_part;
    float* slabs; int64_t partials;
} dgll_edge_proj_desc;
int dgll_hip_edge_proj_pass(void* stream, const dgll_edge_proj_desc* d);

/* ---- Gaussian-mixture edge weights (MoNet / DGL's GMMConv): three passes behind one entry point (csrc/gmm.hip) -------------------------
 * Every entry e of a CSR matrix A [n_dst x n_src] (rectangular allowed, duplicate entries are separate edges) carries `dim`
 * pseudo-coordinates pseudo[e, :] (fp32, pitch ld_pseudo >= dim in elements, 4-byte alignment is enough), in A's entry order.  With
 * mu and inv_sigma fp32 [K, dim], contiguous:
 *     w_k(e) = exp(-0.5 * sum_d ((pseudo[e, d] - mu[k, d]) * inv_sigma[k, d])^2)      fp32, d ascending, ONE device function in every
 *                                                                                      pass: u == mu gives exactly 1, an exponent
 *                                                                                      below 2^-149 exactly 0
 *     Z[i, k, :] = scale[i] * sum_{e = (j -> i)} w_k(e) * X[j, :]                      Z: [n_dst, K * F], kernel-major blocks of width F
 *   DGLL_GMM_EXPAND    rowptr / col = A, n_rows = n_dst, n_cols = n_src.  Reads x [n_src, F] (gathered once per entry into up to
 *                      DGLL_GMM_KERNEL_BLOCK kernels' accumulators; more kernels re-gather x once per block), pseudo at slot e, scale
 *                      (fp32 [n_rows], or NULL: 1); writes out = Z [n_rows, K * F] of `dtype` (zeros for an empty row).
 *   DGLL_GMM_CONTRACT  rowptr / col = A^T with perm (graph.transpose(): A^T's entry -> A's entry), n_rows = n_src, n_cols = n_dst.
 *                      Reads dz [n_dst, K * F] (gathered), pseudo at slot perm[e']; writes out = dX [n_src, F]:
 *                      dX[j] = sum_e sum_k w_k(e) dz[i_e, k, :] (zeros for a source no row references).  scale is not read: the
 *                      caller scales the rows of dz.
 *   DGLL_GMM_PARAM     no rowptr, no col: the nnz entries are streamed.  Reads p fp32 [nnz, ld_p], ld_p = K rounded up to 4, 16-byte
 *                      aligned (p[e, k] = <x[j_e], dz[i_e, k, :]>: dgll_hip_typed_spmm_pass's DGLL_TYPED_EDGE_DOTS with B = K), and
 *                      pseudo.  With u = pseudo[e], s = inv_sigma: writes grad_pseudo[e, d] = sum_k p_k w_k * (-(u_d - mu_kd) s_kd^2)
 *                      (fp32 [nnz, ld_grad_pseudo], or NULL: not wanted) and one fp32 slab [2, K, dim] per workgroup, `partials`
 *                      workgroups taking the entries grid-stride: slabs[w, 0] the share of grad_mu = sum_e p_k w_k (u_d - mu_kd) s_kd^2,
 *                      slabs[w, 1] that of grad_inv_sigma = -sum_e p_k w_k (u_d - mu_kd)^2 s_kd.  Every element of every slab is
 *                      written; the caller sums the slabs in slab order.  dtype is checked and otherwise unused.
 * 1 <= dim <= DGLL_GMM_MAX_DIM, 1 <= K <= DGLL_GMM_MAX_KERNELS; mu and inv_sigma are staged in LDS once per workgroup.  Matrices of
 * `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation), pitches ld_* in elements: whole 16-byte vectors, 16-byte aligned bases; F a
 * multiple of the vector width.  Rows wider than 64 lane vectors are cut into column blocks; rows longer than DGLL_GMM_LONG_ROW
 * entries are swept by a whole workgroup.  col and perm values used for addressing are clamped.  No atomics: two runs give the same
 * bits.  No pass allocates, synchronises or reads anything back: the calls can be captured into a graph.                           */
enum { DGLL_GMM_EXPAND = 0, DGLL_GMM_CONTRACT = 1, DGLL_GMM_PARAM = 2 };
#define DGLL_GMM_LONG_ROW 256
#define DGLL_GMM_MAX_DIM 8
#define DGLL_GMM_MAX_KERNELS 64
#define DGLL_GMM_KERNEL_BLOCK 8
#define DGLL_GMM_MAX_PARTIALS 2048
typedef struct dgll_gmm_desc {
    int pass; int dtype; int K; int dim;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int64_t F;
    const float* scale;
    const float* pseudo; int64_t ld_pseudo;
    const float* mu; const float* inv_sigma;
    const void* x; int64_t ld_x;
    const void* dz; int64_t ld_dz;
    void* out; int64_t ld_out;
    const float* p; int64_t ld_p;
    float* grad_pseudo; int64_t ld_grad_pseudo;
    float* slabs; int64_t partials;
} dgll_gmm_desc;
int dgll_hip_gmm_pass(void* stream, const dgll_gmm_desc* d);

/* ---- Per-column soft aggregation (DeeperGCN: PyG's GENConv, SoftmaxAggregation, PowerMeanAggregation) and its exact backward; three
 * passes behind one entry point (csrc/soft_agg.hip).  Entry k of row i of A (rowptr / col, [n_dst x n_src], rectangular allowed, edge
 * values are not read) is the edge j = col[k] -> i and e[k] its row (optional: e == NULL reads none, in every pass); duplicate entries
 * are separate edges.  For every column independently, with theta = *theta (t or p: ONE fp32 value in device memory, read by the
 * kernels and never by the host), x [n_src, F], e [nnz, F] and g = grad_out [n_dst, F]:
 *     m_k = relu(x[j] + e[k]) + eps        gate_k = (x[j] + e[k] > 0)      the fp32 sum of the two STORED values, ONE device function
 *                                                                          in every pass: relu and gates agree bit for bit
 *   DGLL_SOFT_AGG_SOFTMAX   a_k = exp(t m_k - lse_i), lse_i = log sum_k exp(t m_k), out_i = sum_k a_k m_k      (online, exp2 form, one
 *                           running maximum PER COLUMN)
 *                           d out_i / d m_k = a_k (1 + t (m_k - out_i))      (semi_grad != 0: a_k alone)
 *                           d out_i / d t   = sum_k a_k (m_k^2 - out_i^2)
 *   DGLL_SOFT_AGG_POWER     mc_k = min(m_k, 100), S_i = sum_k mc_k^p, out_i = (S_i / deg_i)^(1/p)      (powers as exp2(p log2 mc))
 *                           d out_i / d m_k = (out_i / S_i) mc_k^(p-1)       (0 where m_k > 100)
 *                           d out_i / d p   = (out_i / p) sum_k (mc_k^p / S_i) (ln mc_k - ln out_i)
 *   DGLL_SOFT_AGG_FORWARD  rowptr / col = A (n_rows = n_dst, n_cols = n_src).  Reads x (gathered), e at slot k; writes out [n_rows, F] of
 *                          `dtype` and the fp32 row statistics stats [n_rows, 2 F]: SOFTMAX {lse | out}, POWER {out | S}, the unrounded
 *                          values.  A row without entries: zeros in both.  Nothing per edge is written.
 *   DGLL_SOFT_AGG_ROWS     rowptr / col = A.  Reads grad_out and stats (held), x (gathered), e at slot k.  Writes, when grad_e is
 *                          non-NULL (e is then required), grad_e[k] = g_i (d out_i / d m_k) gate_k: one store per entry, no reduction;
 *                          and, when grad_theta is non-NULL, the scalar gradient sum over rows and columns of g (d out / d theta):
 *                          at most n_partials workgroups take the row tiles grid-stride, each reduces its lanes in a fixed order into
 *                          ONE fp32 of partials (n_partials * ceil(F / 64 vectors) floats, required then), and a second small kernel
 *                          sums the partials in workgroup order into grad_theta[0].  At least one of the two.  SOFTMAX with semi_grad
 *                          has no scalar gradient: grad_theta must be NULL.
 *   DGLL_SOFT_AGG_COLS     rowptr / col = A^T with perm, A^T's entry k' -> A's entry (graph.transpose(); n_rows = n_src, n_cols = n_dst;
 *                          perm is required when e is given).  Reads x (held), grad_out and stats (gathered at i = col[k']), e at slot
 *                          perm[k']; writes grad_x [n_rows, F] (zeros for a source no row references).
 * eps >= 0.  Operands a pass does not read may be NULL and are not dereferenced.  nnz: the rows of e / grad_e (perm values are clamped
 * to [0, nnz), col values used for addressing to [0, n_cols)).  Matrices of `dtype` (DGLL_F32 / DGLL_BF16, fp32 accumulation) but for
 * the fp32 stats; pitches ld_* in elements, each its own: whole 16-byte vectors >= F (stats: >= 2 F), 16-byte aligned bases; columns
 * behind F are never read into a result and never written.  F a positive multiple of the vector width (4 fp32 / 8 bf16 columns);
 * widths past 64 vectors go to column blocks.  Rows longer than DGLL_SOFT_AGG_LONG_ROW entries are swept by a whole workgroup and,
 * where there is a row reduction, merged through LDS in group order (SOFTMAX: with a per-column rescale).  No atomics: two runs give
 * the same bits, grad_theta included.  No pass allocates, synchronises or reads anything back: the calls can be captured into a
 * graph.  n_rows == 0 launches nothing and writes nothing, grad_theta included.                                                      */
enum { DGLL_SOFT_AGG_FORWARD = 0, DGLL_SOFT_AGG_ROWS = 1, DGLL_SOFT_AGG_COLS = 2 };
enum { DGLL_SOFT_AGG_SOFTMAX = 0, DGLL_SOFT_AGG_POWER = 1 };
#define DGLL_SOFT_AGG_LONG_ROW 256
#define DGLL_SOFT_AGG_MAX_PARTIALS 1024
typedef struct dgll_soft_agg_desc {
    int pass; int dtype; int mode; int semi_grad;
    const int64_t* rowptr; const int32_t* col; const int64_t* perm; int64_t n_rows; int64_t n_cols; int64_t nnz;
    int64_t F; float eps;
    const float* theta;
    const void* x; int64_t ld_x;
    const void* e; int64_t ld_e;
    const void* grad_out; int64_t ld_grad_out;
    void* out; int64_t ld_out;
    float* stats; int64_t ld_stats;
    void* grad_x; int64_t ld_grad_x;
    void* grad_e; int64_t ld_grad_e;
    float* partials; int64_t n_partials;
    float* grad_theta;
} dgll_soft_agg_desc;
int dgll_hip_soft_agg_pass(void* stream, const dgll_soft_agg_desc* d);

/* ---- Exact k nearest neighbours inside segments (DGL's knn_graph / segmented_knn_graph; the graph of Dynamic Graph CNN), one launch
 * (csrc/knn.hip).
 *   Inputs    x [n, D] of `dtype` (DGLL_F32 / DGLL_BF16) on a row pitch ld_x >= D in elements; whatever lies behind column D of a row
 *             is never read into a result.  16-byte loads are used when x is 16-byte aligned and the pitch a whole number of 16-byte
 *             vectors (the row's pitch is then addressable up to the end of the vector that holds column D - 1), scalar loads otherwise.
 *             seg_ptr int64 [n_segs + 1], ascending, cuts the rows into n_segs contiguous segments; empty segments are allowed; a row
 *             that no segment covers gets no entries.  k >= 1; exclude_self is a flag.
 *   Distance  d(i, j) = sum over c = 0 .. D-1 of (x[i,c] - x[j,c])^2 in fp32, on the inputs converted exactly to fp32: the DIFFERENCE
 *             form (never |xi|^2 - 2 xi.xj + |xj|^2, whose cancellation changes which neighbour wins).  A NaN distance sorts as +inf.
 *   Output    row i of segment s gets deg_i = min(k, size(s) - (exclude_self ? 1 : 0)) entries, written at out_rowptr[i] (int64 [n + 1],
 *             an INPUT: the caller knows deg_i from the segment sizes): the deg_i candidates j of its own segment with the smallest
 *             (d, j) in lexicographic order, in that order -- among equal fp32 distances the smaller index wins.  With exclude_self the
 *             candidate j == i is skipped by INDEX, not by distance: a duplicate point is still a neighbour.  out_col int32 [out_nnz]
 *             receives global row ids, out_dist fp32 [out_nnz] (may be NULL) the distances; a slot outside [0, out_nnz) is not written.
 *   Limits    1 <= k <= DGLL_KNN_MAX_K, 1 <= D <= DGLL_KNN_MAX_D, n < 2^31; anything else returns DGLL_ERR_INVALID and names the limit.
 *             Every argument check happens on the host before any launch.
 * Workgroups take tiles of DGLL_KNN_QUERY_TILE consecutive rows (one lane per query) and stream the segment's rows through LDS in tiles of
 * DGLL_KNN_CAND_TILE rows.  No atomics, no scratch memory, nothing of size n x n or n x segment anywhere: two runs give the same bits.
 * Nothing is allocated, synchronised or read back: the call can be captured into a graph.  n == 0, n_segs == 0 or out_nnz == 0 launch
 * nothing.                                                                                                                            */
#define DGLL_KNN_MAX_K 64
#define DGLL_KNN_MAX_D 256
#define DGLL_KNN_QUERY_TILE 256
#define DGLL_KNN_CAND_TILE 32
int dgll_hip_knn(void* stream, const void* x, int64_t ld_x, int dtype, int64_t n, int64_t D, const int64_t* seg_ptr, int64_t n_segs,
                 int k, int exclude_self, const int64_t* out_rowptr, int32_t* out_col, float* out_dist, int64_t out_nnz);

#ifdef __cplusplus
}
#endif
#endif /* DGLL_HIP_H */
