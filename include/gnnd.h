/*
 * gnnd.h — C ABI of libgnnd.so, the MI355X-native (gfx950) GNN belief-propagation decoder.
 *
 * This is the drop-in boundary for the reference's hot path (paths relative to
 * /root/reference/GNN-decode/):
 *
 *   MessagePassing.propagate()   quantum/decoder_v2_4.py:85-148, quantum/QGNNI.py:54-116,
 *                                quantum/BP.py:54-124, classical/CGNNI.py:52-112,
 *                                classical/BP.py:52-123       -> gnnd_propagate_tiled / _generic
 *   scatter_ (PyG-1.x)           quantum/decoder_v2_4.py:34-51 -> aggregation inside the above
 *   GNNI.forward() T-loop        classical/CGNNI.py:259-284, classical/BP.py:239-259,
 *     + update() MLPs + readout  quantum/BP.py:199-219, quantum/QGNNI.py:228-252,
 *                                quantum/decoder_v2_4.py:272-294 -> gnnd_decode
 *   H.to_sparse()._indices()     quantum/decoder_v2_4.py:164-165 -> gnnd_graph_create
 *
 * Conventions
 *   - Plain pointers and sizes only; no framework types.  Every pointer named d_* is DEVICE
 *     memory owned by the caller; h_* is host memory.  Kernels never allocate.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No function that
 *     takes a stream synchronises the host, so every such call is graph-capturable.
 *   - Every function returns a gnnd_status; nothing throws or aborts.
 *   - Batch layout is the reference's PyG collation (graph-major): codeword b owns node rows
 *     [b*N, (b+1)*N) with N = V + C (variable rows first, then check rows) and edge rows
 *     [b*E, (b+1)*E) in the single-graph edge order (sorted by (v, c)).
 */
#ifndef GNND_H
#define GNND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNND_VERSION 1

typedef enum gnnd_status {
    GNND_OK = 0,
    GNND_ERR_INVALID_ARG = 1,   /* bad pointer / size / enum value                     */
    GNND_ERR_HIP = 2,           /* a HIP runtime call failed (see gnnd_last_hip_error)  */
    GNND_ERR_UNSUPPORTED = 3,   /* valid request this build does not implement         */
    GNND_ERR_GRAPH = 4,         /* edge list is not a valid Tanner graph                */
    GNND_ERR_ALLOC = 5          /* device allocation failed (graph creation only)       */
} gnnd_status;

/* GNND_BF16 (gnnd_decode of CGNNI / CBP only): x and out stored as bf16 in HBM, weights
 * fp32 (gnnd_prepare_weights with GNND_F32), every operation in fp32 — BASELINE config 2's
 * "bf16" storage mode.                                                                      */
typedef enum gnnd_dtype { GNND_F32 = 0, GNND_F64 = 1, GNND_BF16 = 2 } gnnd_dtype;

/* `flow` of MessagePassing (quantum/decoder_v2_4.py:73-74,89):
 *   SOURCE_TO_TARGET: aggregate at edge_index[0] (variable nodes)  = v->c message
 *   TARGET_TO_SOURCE: aggregate at edge_index[1] (check nodes)     = c->v message     */
typedef enum gnnd_flow { GNND_SOURCE_TO_TARGET = 0, GNND_TARGET_TO_SOURCE = 1 } gnnd_flow;

/* `aggr` of MessagePassing (quantum/decoder_v2_4.py:70-71); PyG-1.x scatter_ rules. */
typedef enum gnnd_aggr { GNND_AGGR_ADD = 0, GNND_AGGR_MEAN = 1, GNND_AGGR_MAX = 2 } gnnd_aggr;

/* Which reference script's propagate body (the scripts each carry their own copy):
 *   V24    quantum/decoder_v2_4.py:132-144  c->v tanh(x/2); both flows cat extra[idx_j] (F=2)
 *   QGNNI  quantum/QGNNI.py:101-112         c->v tanh(x/2), cat (F=2); v->c + extra (F=1)
 *   QBP    quantum/BP.py:101-119            c->v log-domain BP with syndrome; v->c + extra
 *   CGNNI  classical/CGNNI.py:99-108        c->v tanh(x/2); + post (if non-NULL) (F=1)
 *   CBP    classical/BP.py:99-119           c->v log-domain BP; v->c + extra (F=1)
 *   NBP    quantum/neural_BP.py:108-131     c->v log-domain BP with syndrome, no +-10
 *                                           pre-clamp, p clamp 1 - 1e-15; v->c cat (F=2)
 *   V10    quantum/decoder_v1_0.py:109-131  c->v as NBP; v->c + extra (F=1)
 *   V30    quantum/decoder_v3_0.py:106-118  no pre-op on either side (edge states
 *                                           aggregated raw); both flows cat (F=2)
 *   V22    quantum/decoder_v2_2.py:133-160  the NBP body (the script's propagate is
 *                                           neural_BP.py's); decoder only: gnnd_propagate_*
 *                                           take NBP for it                              */
typedef enum gnnd_variant {
    GNND_V24 = 0, GNND_QGNNI = 1, GNND_QBP = 2, GNND_CGNNI = 3, GNND_CBP = 4,
    GNND_NBP = 5, GNND_V10 = 6, GNND_V30 = 7, GNND_V22 = 8
} gnnd_variant;

/* Whole-decoder models for gnnd_decode (same enumerators as gnnd_variant). */
typedef gnnd_variant gnnd_model;

typedef struct gnnd_graph gnnd_graph;   /* opaque; device-resident single-codeword graph */

/* ---- graph --------------------------------------------------------------------------
 * Build the single-codeword Tanner graph from its edge list, i.e. the reference's
 * `H.to_sparse()._indices()` of H[V, C] (row 0 = variable, row 1 = check), which must be
 * sorted by (v, c) with no duplicates.  Replaces the per-batch int64 edge_index reads of
 * the reference (quantum/decoder_v2_4.py:164-165, 277) with a cached CSR/CSC.          */
int gnnd_graph_create(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                      int32_t num_var, int32_t num_chk, gnnd_graph** out);
int gnnd_graph_destroy(gnnd_graph* g);
/* Host-only: build every table gnnd_graph_create would upload and check its structural
 * invariants (slot plans, padded / x-augmented message layouts); no device needed.
 * h_report4 = {slot plans checked, layouts checked, edges, invariant failures}.          */
int gnnd_graph_validate_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int32_t* h_report4);
/* dims[0..5] = V, C, E, N, max variable degree, max check degree */
int gnnd_graph_dims(const gnnd_graph* g, int32_t* h_dims6);
/* Connected components the graph was split into (1 = not split).  A Tanner graph made of
 * 2..8 equal-shaped components, each a contiguous variable range with a contiguous check
 * range (the toric code of quantum/error_generate.py:39-132: its X and Z halves), is decoded
 * and trained by decoder_v2_4 with every component of a codeword in its own workgroup (the
 * components share no edge, so nothing is exchanged; results are the same as whole-graph
 * decoding up to fp32 summation order).  Set GNND_NO_SPLIT=1 to disable.                  */
int gnnd_graph_components(const gnnd_graph* g, int32_t* h_ncomp);
int gnnd_graph_set_split(gnnd_graph* g, int32_t enable);   /* 0: decode / train it whole */

/* Check on the device that a batched edge_index (int64, rows 0/1 at d_edge_index and
 * d_edge_index + row_stride, num_batched_edges columns) is the single graph tiled over
 * `batch` codewords with node offset b*N and check ids shifted by `chk_shift` (V after
 * GNNI.forward's shift, 0 before it).  Writes 1 (tiled) / 0 to *d_flag (device int32). */
int gnnd_check_tiled(const gnnd_graph* g, const int64_t* d_edge_index, int64_t row_stride,
                     int64_t num_batched_edges, int64_t batch, int64_t chk_shift,
                     int32_t* d_flag, void* stream);

/* ---- operator: one propagate() call ---------------------------------------------------
 * Tiled fast path (aggr ADD or MAX).  d_msg [B*E] (the per-edge `x` kwarg), d_extra [B*N]
 * (the `extra`/`post` argument; may be NULL only for CGNNI), d_out [B*E, F] row-major with
 * F = gnnd_propagate_width(variant, flow).  dtype selects float/double for all three.    */
int gnnd_propagate_width(int variant, int flow);
int gnnd_propagate_tiled(const gnnd_graph* g, int variant, int flow, int aggr, int dtype,
                         const void* d_msg, const void* d_extra, void* d_out, int64_t batch,
                         void* stream);

/* Generic path for an arbitrary edge_index (any aggr, including the reference's literal
 * leave-one-out `mean`).  Uses float atomics for the scatter, so sums are order-dependent
 * in the last bits.  d_workspace must hold gnnd_propagate_generic_workspace() bytes.    */
int gnnd_propagate_generic_workspace(int variant, int flow, int aggr, int dtype,
                                     int64_t num_edges, int64_t dim_size, int64_t* h_bytes);
int gnnd_propagate_generic(int variant, int flow, int aggr, int dtype,
                           const int64_t* d_edge_index, int64_t row_stride, int64_t num_edges,
                           const void* d_msg, const void* d_extra, int64_t dim_size,
                           void* d_out, void* d_workspace, int64_t workspace_bytes,
                           void* stream);

/* Backward of one propagate call w.r.t. d_msg (training; aggr ADD, every variant).
 * d_grad_out is [B*E, F] like d_out, d_grad_msg [B*E].  d_extra is the forward's `extra`
 * (the syndrome sets the sign of the BP check step; may be NULL except for the quantum BP
 * bodies QBP/NBP/V10 with flow TARGET_TO_SOURCE).  The c->v BP bodies recompute their
 * forward and apply torch's autograd rules (clamp passes the gradient on [lo, hi], abs
 * uses sign(t), tanh 1 - t^2).  The generic form needs a workspace of
 * gnnd_propagate_generic_bwd_workspace() bytes.                                           */
int gnnd_propagate_tiled_bwd(const gnnd_graph* g, int variant, int flow, int aggr, int dtype,
                             const void* d_msg, const void* d_extra, const void* d_grad_out,
                             void* d_grad_msg, int64_t batch, void* stream);
int gnnd_propagate_generic_bwd_workspace(int variant, int flow, int aggr, int dtype,
                                         int64_t num_edges, int64_t dim_size, int64_t* h_bytes);
int gnnd_propagate_generic_bwd(int variant, int flow, int aggr, int dtype,
                               const int64_t* d_edge_index, int64_t row_stride,
                               int64_t num_edges, const void* d_msg, const void* d_extra,
                               const void* d_grad_out, int64_t dim_size, void* d_grad_msg,
                               void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- fused T-iteration decoder --------------------------------------------------------
 * Runs the whole GNNI.forward (m0 = 0, T iterations of both half-steps, residual, readout)
 * for `batch` codewords in one launch; messages never leave the CU.
 *   d_x   [B*N]   node features (priors/LLRs at variable rows, syndrome at check rows)
 *   d_out [B*V]   P(bit = 1)  (sigmoid(-readout), clamped for the classical models)
 *         V30: [2*B*N], the reference's two-output readout (quantum/decoder_v3_0.py:
 *         274-290): [0, B*N) = sigmoid(-(mlp(S_v) + x)) per node (checks: S = 0),
 *         [B*N, 2*B*N) = sigmoid(-mlp(S_c(m_p))) per node (variables: S = 0), m_p = the
 *         v->c edge states of the last iteration
 *         V22: [iters*B*V], the reference's per-iteration readout list (quantum/
 *         decoder_v2_2.py:333-347): block t = sigmoid(-(S_v(m_t W) + S_v(x W_pr))) after
 *         iteration t (register-resident plans only: GNND_ERR_UNSUPPORTED otherwise)
 *   d_w   weights in `dtype` as produced by gnnd_prepare_weights from the packed
 *         state_dict layout below (gnnd_weights_count elements, same count after prepare):
 *     CGNNI: ggc2.mlp2 {W1[10], b1[10], W2[10], b2}, mlp {W1[10], b1[10], W2[10], b2}  = 62
 *     QGNNI: ggc2.mlp  {W1[10], b1[10], W2[10], b2}, mlp {same}                          = 62
 *     V24:   ggc1.mlp  {W1[:,0][128], W1[:,1][128], b1[128], W2[128], b2},
 *            ggc2.mlp  {W1[128], b1[128], W2[128], b2}, mlp {W1[128], b1[128], W2[128], b2}
 *                                                                                    = 1283
 *     CBP, QBP: none (d_w may be NULL)
 *     NBP (quantum/neural_BP.py, per-edge weights in reference edge order, T = iters):
 *            for t < T {layers[2t].W[E], layers[2t].W_p[E]}, then W[E], W_p[E], alpha
 *                                                                          = 2 E T + 2 E + 1
 *     V10 (quantum/decoder_v1_0.py): for t < T {layers[2t+1].W[E]}, then alpha  = E T + 1
 *     V22 (quantum/decoder_v2_2.py, weights shared by the 8 edge types of H_prime): the NBP
 *            layout with every type weight expanded per edge, w[e] = W[type(e)]:
 *            for t < T {layers[2t].W[type][E], layers[2t].W_p[type][E]}, then
 *            W[type][E], W_pr[type][E], sigmoid(weight)               = 2 E T + 2 E + 1
 *     V30 (quantum/decoder_v3_0.py, GRU edge states; the unused ggc1.mlp2/rnn2 and
 *            ggc2.mlp1/rnn1 are not passed):
 *            ggc1.mlp1 {W1[10][2] row-major, b1[10], W2[10], b2},
 *            ggc1.rnn1 {weight_ih[3], weight_hh[3], bias_ih[3], bias_hh[3]} (gates r, z, n),
 *            ggc2.mlp2 {same as ggc1.mlp1}, ggc2.rnn2 {same as rnn1},
 *            mlp {W1[10], b1[10], W2[10], b2}                                            = 137
 * gnnd_prepare_weights converts that layout into the kernel layout (for the fp32 V24
 * kernel the softplus layers are rescaled to base 2: layer-1 rows * log2(e), layer-2
 * weights * ln(2); V24 appends the check-MLP table and fp32 CGNNI / QGNNI the message
 * MLP's piecewise-linear table, gnnd_prepared_weights_count elements; every other model/dtype
 * is a plain copy).  Call it once per weights.
 * gnnd_weights_count is the graph-independent count (GNND_ERR_UNSUPPORTED for NBP/V10/V22,
 * whose packed layout is passed to gnnd_decode as is, without preparation);
 * gnnd_decode_weights_count covers every model for a graph and iteration count.         */
int gnnd_weights_count(int model, int64_t* h_count);
int gnnd_decode_weights_count(const gnnd_graph* g, int model, int32_t iters, int64_t* h_count);
int gnnd_prepare_weights(int model, int dtype, const void* d_w, void* d_prepared,
                         void* stream);
/* Elements of gnnd_prepare_weights' output: gnnd_weights_count, except V24 (7 264, fp32 and
 * fp64): the 1 283 weights (fp32: base-2 rescaled), then the check-MLP table
 * (gnnd_v24_check_mlp_table) the decoder and training forward read, then a 12-element
 * channel-prior header (0 tables; see gnnd_prepare_weights_priors).  CGNNI / QGNNI: 62, the plain
 * weights, in the default build (fp32 builds with the message MLP's piecewise-linear table
 * compiled in append it: 328).  Ask gnnd_prepared_weights_count, do not hard-code.  gnnd_decode
 * needs this prepared buffer, not the plain weights (so does gnnd_train_fwd for V24).         */
int gnnd_prepared_weights_count(int model, int dtype, int64_t* h_count);
int gnnd_decode(const gnnd_graph* g, int model, int dtype, const void* d_w, const void* d_x,
                void* d_out, int64_t batch, int32_t iters, void* stream);

/* Channel-prior tables (fp64 decoder_v2_4).  The variable-side MLP ggc1.mlp (Linear(2,128) ->
 * Softplus -> Linear(128,1), quantum/decoder_v2_4.py:237-239, :253-255) takes (S_v - m_e, x_v);
 * the reference's inputs carry one prior LLR x_v = log((1-p)/p) per codeword, p drawn from a
 * short list (quantum/error_generate.py:252-260).  gnnd_prepare_weights_priors = gnnd_prepare_weights
 * plus, for each of the n_priors values h_priors[] (host fp64, <= 64; the exact x_v bits the
 * inputs will carry), tanh(MLP/2) -- the check step's pre-op of its output -- tabulated over
 * |S_v - m_e| <= 32 (64-byte cells: degree-7 Taylor polynomials about j/16; the readout MLP's
 * about j/32; up to 3 units crossing torch's Softplus threshold inside a cell are stored aside and
 * their jumps added exactly; a cell whose MLP remainder bound exceeds 1e-13, whose tanh series
 * misses tanh(P/2) of the MLP's own cell polynomial P at a cell edge by more than 2e-14, or that
 * holds more crossings is marked invalid and its points take the 128 units), into a buffer of
 * gnnd_prepared_weights_count_priors elements.  gnnd_decode
 * (fp64 V24, batches decoded one wave per item group) then reads a codeword's table where its
 * x_v equals a registered prior bit for bit and evaluates the 128 units elsewhere (other priors,
 * |S_v - m_e| > 32), and the readout MLP from one more table (n_priors > 0).  The tables
 * depend on the weights: gnnd_train_update and
 * gnnd_prepare_weights reset the count to 0.  Other models/dtypes: n_priors must be 0.        */
int gnnd_prepared_weights_count_priors(int model, int dtype, int32_t n_priors, int64_t* h_count);
int gnnd_prepare_weights_priors(int model, int dtype, const void* d_w, void* d_prepared,
                                const double* h_priors, int32_t n_priors, void* stream);
/* The same tables with no host round trip: the prior list is found and read on the device, all
 * on `stream` (memsets and kernel launches only: no host read, no synchronisation, no blocking
 * copy), so the pair can run inside a stream capture and on batches whose p list changes.
 * gnnd_v24_scan_priors (fp64 only: other dtypes GNND_ERR_UNSUPPORTED) reads each codeword's
 * FIRST variable input, d_x[b * N] -- the element gnnd_decode keys a codeword's table on -- and
 * writes the distinct values, compared bit for bit as the decoder does, NaN skipped, ASCENDING by
 * value into d_priors[0 .. count), zeros into d_priors[count .. 64), and d_status = {count, 0}
 * (device fp64 [64] and int32 [2]).  More than 64 distinct values: d_priors all zero and
 * d_status = {0, 1}; no tables are built and the decode stays exact through the 128 units.  The
 * result is a pure function of d_x (the same bits on every launch).
 * gnnd_prepare_weights_priors_dev (fp64 V24 only: GNND_ERR_UNSUPPORTED otherwise) =
 * gnnd_prepare_weights plus the tables of d_priors[0 .. d_status[0]) and the readout table, the
 * same bits gnnd_prepare_weights_priors builds from that list.  The host does not know the
 * count, so d_prepared must hold the 64-prior layout: prepared_capacity (elements) >=
 * gnnd_prepared_weights_count_priors(.., 64), else GNND_ERR_INVALID_ARG.  Count 0: the buffer is
 * gnnd_prepare_weights' (header 0, no tables).                                              */
int gnnd_v24_scan_priors(const gnnd_graph* g, int dtype, const void* d_x, int64_t batch,
                         double* d_priors, int32_t* d_status, void* stream);
int gnnd_prepare_weights_priors_dev(int model, int dtype, const void* d_w, void* d_prepared,
                                    int64_t prepared_capacity, const double* d_priors,
                                    const int32_t* d_status, void* stream);
/* The tables as the decoder evaluates them, for tests: d_y[i] = tanh(ggc1.mlp(d_u[i], d_x[i]) / 2)
 * (the prior tables hold the check step's pre-op tanh(m/2) of ggc1's output directly, as degree-7
 * series composed from the MLP's; quantum/decoder_v2_4.py:135-136) and
 * d_hit[i] = 1 where a table covers the point, else d_hit[i] = 0 and d_y[i] untouched
 * (d_w = prepared fp64 V24 weights with tables; device fp64 d_u, d_x, d_y [n], int32 d_hit).
 * The prepared tables end with one for the readout MLP (mlp, quantum/decoder_v2_4.py:291, over
 * |m| <= 32, no prior): d_x = NULL evaluates that one, d_y[i] = mlp(d_u[i]).                 */
int gnnd_v24_var_mlp_table(const void* d_w, const void* d_u, const void* d_x, void* d_y,
                           int32_t* d_hit, int64_t n, void* stream);

/* decoder_v2_4's check-side MLP (ggc2.mlp: Linear(1,128) -> Softplus -> Linear(128,1),
 * quantum/decoder_v2_4.py:241-243, :253-257) as the fp64 decoder evaluates it: its input
 * u = S_c(tanh(m/2)) - tanh(m_e/2) lies in [-R, R], R = max check degree - 1, so the fp64
 * prepared weights carry it tabulated (degree-11 Taylor polynomials about j/8, |j/8| <= 31;
 * gnnd_prepare_weights and gnnd_train_update build the table) and the decoder reads the table
 * instead of the 128 hidden units.  This evaluates the same table at d_u [n] (fp64, inside
 * [-R, R]) into d_y [n]; d_w = PREPARED fp64 V24 weights.  *d_ok (device int32) = 1 when the
 * table is valid for this graph -- the decoder uses it -- or 0 (d_y untouched) when a unit's
 * pre-activation crosses torch's Softplus threshold 20 for some u in [-R, R], the Taylor
 * remainder bound exceeds 1e-13, or R > 31 (the decoder then evaluates the units).          */
int gnnd_v24_check_mlp_table(const gnnd_graph* g, const void* d_w, const void* d_u, void* d_y,
                             int64_t n, int32_t* d_ok, void* stream);

/* Codewords per workgroup the decoder would use (for roofline bookkeeping). */
int gnnd_decode_tile(const gnnd_graph* g, int model, int dtype, int32_t* h_cw_per_block,
                     int32_t* h_lds_bytes);
/* Full launch plan: h_plan[0] codewords per workgroup, [1] LDS bytes per workgroup,
 * [2] kernel (0 = streaming decode_kernel, 1 = register-resident decode_resident_kernel),
 * [3] work items per lane (resident kernel; 0 otherwise), [4] variable-sum group of the
 * resident kernel's message layout (vars per wave step padded to one degree; 1 = identity
 * layout; 0 for the streaming kernel).  h_plan holds 5 ints. */
int gnnd_decode_plan(const gnnd_graph* g, int model, int dtype, int32_t* h_plan);

/* ---- fused training step (decoder_v2_4) ------------------
 * gnnd_train_fwd = gnnd_decode (same prepared weights, same output) that also writes the
 * training tape (gnnd_train_tape_bytes bytes of d_tape): per iteration and edge the
 * v->c MLP input, the tanh output and the c->v MLP input, plus the final messages.
 * gnnd_train_bwd turns d loss / d out [B*V] into d loss / d weights [1283] (V24) in the PLAIN
 * packed layout of gnnd_weights_count (d_w is that plain layout, not the prepared one):
 * reverse mode through all T iterations and the readout in one launch (+ a fixed-order
 * reduction of per-workgroup partials in d_workspace, gnnd_train_bwd_workspace bytes).
 * Models: V24 (quantum/decoder_v2_4.py:260-294, fp32/fp64), V30 (quantum/decoder_v3_0.py:
 * 245-290, fp32/fp64; d_out / d_grad_out are the two readout tensors [2][B*N]), and fp64 NBP
 * (quantum/neural_BP.py:263-314), V22 (quantum/decoder_v2_2.py:299-347; d_out /
 * d_grad_out every layer's readout [T][B*V]) and V10 (quantum/decoder_v1_0.py:263-313)
 * whose gradient is w.r.t. the per-edge tables of their packed layout (NBP/V22 2 E T + 2 E + 1
 * values, V10 E T + 1), CGNNI (classical/CGNNI.py:248-284) and
 * QGNNI (quantum/QGNNI.py:217-252), fp32/fp64, gradient w.r.t. their 62 packed weights (the
 * forward writes its own tape: every iteration's tanh outputs and the readout inputs; d_out
 * is its prediction, not gnnd_decode's register-resident one bit for bit).  The other models
 * train through gnnd_propagate_*_bwd.  gnnd_train_workspace_bytes sizes the workspace of every model
 * (gnnd_train_bwd_workspace, which has no iteration count, only V24 and V30).             */
int gnnd_train_tape_bytes(const gnnd_graph* g, int model, int dtype, int64_t batch,
                          int32_t iters, int64_t* h_bytes);
int gnnd_train_fwd(const gnnd_graph* g, int model, int dtype, const void* d_w, const void* d_x,
                   void* d_out, void* d_tape, int64_t batch, int32_t iters, void* stream);
int gnnd_train_bwd_workspace(const gnnd_graph* g, int model, int dtype, int64_t batch,
                             int64_t* h_bytes);
int gnnd_train_workspace_bytes(const gnnd_graph* g, int model, int dtype, int64_t batch,
                               int32_t iters, int64_t* h_bytes);
int gnnd_train_bwd(const gnnd_graph* g, int model, int dtype, const void* d_w, const void* d_x,
                   const void* d_out, const void* d_grad_out, const void* d_tape,
                   void* d_grad_w, void* d_workspace, int64_t workspace_bytes, int64_t batch,
                   int32_t iters, void* stream);
/* The reverse pass without its reduction: leaves gnnd_train_bwd_rows() per-workgroup
 * gradient rows [rows][n] (n = the model's weights: V24 1283, V30 137, CGNNI/QGNNI 62,
 * NBP/V22 2ET + 2E + 1, V10 ET + 1) in d_workspace, for gnnd_train_update (V24, V30, CGNNI, QGNNI) to
 * reduce (fused with
 * the optimizer).  On a split graph (gnnd_graph_components > 1) every component of a
 * codeword runs in its own workgroup.                                                     */
int gnnd_train_bwd_rows(const gnnd_graph* g, int model, int dtype, int64_t batch,
                        int64_t* h_rows);
int gnnd_train_bwd_partial(const gnnd_graph* g, int model, int dtype, const void* d_w,
                           const void* d_x, const void* d_out, const void* d_grad_out,
                           const void* d_tape, void* d_workspace, int64_t workspace_bytes,
                           int64_t batch, int32_t iters, void* stream);
/* The reverse pass with the syndrome loss of gnnd_syndrome_loss fused in: d_y [B*V] labels,
 * d_logical_mask [V] uint32 = bit l set iff variable v is in logical row l (n_logical <= 32;
 * on a split graph every row's support must lie inside one component).  Each workgroup
 * computes the loss terms of its codeword (component) and their gradient itself; the losses
 * go to d_loss_b [gnnd_train_loss_count(batch)] (one per codeword and component, in codeword
 * order); the batch loss is their sum (gnnd_train_update sums them).  Rows as
 * gnnd_train_bwd_partial.                                                                  */
int gnnd_train_loss_count(const gnnd_graph* g, int64_t batch, int64_t* h_count);
int gnnd_train_bwd_loss_partial(const gnnd_graph* g, int model, int dtype, const void* d_w,
                                const void* d_x, const void* d_out, const void* d_y,
                                const uint32_t* d_logical_mask, int32_t n_logical,
                                int32_t logical_only, const void* d_tape, void* d_loss_b,
                                void* d_workspace, int64_t workspace_bytes, int64_t batch,
                                int32_t iters, void* stream);
/* The same syndrome loss computed in the FORWARD's epilogue instead: gnnd_train_fwd plus
 * d_grad_out [B*V] = d loss / d out and d_loss_b as above (the same terms and summation
 * orders, so the same bits), for gnnd_train_bwd_partial(d_grad_out) to consume.  fp32 V24
 * on its unit-split small-batch plan only (the 16-wave reverse pass then skips its loss
 * phases); returns GNND_ERR_UNSUPPORTED (nothing launched) otherwise.                       */
int gnnd_train_fwd_loss(const gnnd_graph* g, int model, int dtype, const void* d_w,
                        const void* d_x, void* d_out, void* d_tape, const void* d_y,
                        const uint32_t* d_logical_mask, int32_t n_logical, int32_t logical_only,
                        void* d_grad_out, void* d_loss_b, int64_t batch, int32_t iters,
                        void* stream);
/* Fused optimizer epilogue of a decoder_v2_4 training step (one launch):
 *   n_rows > 0: d_grad[i] = fixed-order sum of the rows (d_grad may be NULL: not stored);
 *   n_rows = 0: the gradient is read from d_grad (e.g. after an all-reduce of it);
 *   d_loss_b [batch] non-NULL: *d_loss = fixed-order sum of the per-codeword losses;
 *   d_param non-NULL: gnnd_adam_step's update of the plain packed weights (V24 1283, V30 137,
 *   CGNNI/QGNNI 62; the V30, CGNNI and QGNNI kernel layouts are the plain one) (moments
 *   d_exp_avg / d_exp_avg_sq, device step count *d_step incremented once), then, if
 *   d_prepared is non-NULL, gnnd_prepare_weights' kernel layout of the updated weights into
 *   d_prepared.  d_sync: one device uint32, zero before the first call (the kernel leaves it
 *   zero); it orders the step-count update across the launch's workgroups.
 * Single-rank step: bwd_partial -> update(rows, loss, Adam, prepare).  Data-parallel step:
 * bwd_partial -> update(rows -> d_grad, loss) -> all_reduce(d_grad) -> update(0 rows, Adam). */
int gnnd_train_update(int model, int dtype, const void* d_rows, int64_t n_rows, void* d_grad,
                      const void* d_loss_b, int64_t batch, void* d_loss, void* d_param,
                      void* d_exp_avg, void* d_exp_avg_sq, double* d_step, uint32_t* d_sync,
                      double lr, double beta1, double beta2, double eps, double weight_decay,
                      void* d_prepared, void* stream);

/* ---- training objective ------------------------------------------------
 * Syndrome loss of quantum/decoder_v2_4.py:297-317 (logical_only != 0: the Lambda term of
 * quantum/QGNNI.py:255-290 only) and its gradient, per codeword b of the batch:
 *   d_loss_b[b] = sum_c |sin(pi/2 (H^T (y+p))_c)| + sum_l |sin(pi/2 (Lambda (y+p))_l)|
 *   d_dpred[b*V+v] = d loss_b / d p_v  (torch's |.| rule: sign(0) = 0)
 * d_pred, d_y: [B*V] in dtype; d_logical: int32 [n_logical][V] 0/1 rows of Lambda.  The
 * batch loss of the reference is sum_b d_loss_b[b].  Replaces the reference's LossFunc
 * (its O(B) torch.cat reshape loop and ~30 small autograd kernels per step).            */
int gnnd_syndrome_loss(const gnnd_graph* g, const int32_t* d_logical, int32_t n_logical,
                       int32_t logical_only, int dtype, const void* d_pred, const void* d_y,
                       void* d_loss_b, void* d_dpred, int64_t batch, void* stream);

/* Hard-decision metrics of a decoded batch, replacing the O(B) torch.cat
 * loops of quantum/neural_BP.py:333-348 (FER rule) and the host-side BER counts:
 *   e = (pred > 0.5) xor (y > 0.5) per bit;
 *   d_counts[0] = sum of e (bit errors), [1] = codewords with any bit error,
 *   [2] = codewords with a nonzero residual syndrome H^T e,
 *   [3] = codewords with zero residual syndrome and an odd overlap with some logical row.
 * d_pred, d_y: [B*V] in dtype; d_logical: int32 [n_logical][V] 0/1 rows (n_logical = 0 for
 * classical codes); d_counts: 4 int64 on the device (overwritten).                        */
int gnnd_decision_errors(const gnnd_graph* g, const int32_t* d_logical, int32_t n_logical,
                         int dtype, const void* d_pred, const void* d_y, int64_t* d_counts,
                         int64_t batch, void* stream);

/* ---- OSD-0 post-processing ---------------------------------------------------------------
 * Ordered-statistics decoding of order 0 (the "OSD" of BP+OSD; for the classical codes
 * Fossorier-Lin order-0 reprocessing): from a decoder's soft output, an estimate that satisfies
 * the measured syndrome whenever the syndrome is in the column space of H^T.  Per codeword b,
 * p[v] = d_pred[b*V + v], x = the decoder input in the batch layout above:
 *   target    t[c] = (x[b*N + V + c] < 0)   (quantum inputs carry (-1)^s there, classical 0)
 *   base      GNND_OSD_BASE_ZERO: z = 0, key[v] = p[v]               (the usual quantum form)
 *             GNND_OSD_BASE_HARD: z[v] = (p[v] > 0.5), key[v] = -|p[v] - 0.5|, in `dtype`
 *             a NaN p[v]: key = -inf, z[v] = 0
 *   order     columns by descending key, ties by ascending v (decoder outputs saturate: ties
 *             are common and the rule is part of the contract)
 *   solve     s = t xor H^T z; walk the columns of H^T (C rows) in that order, a column being
 *             a pivot iff some row not yet used holds a 1 in it after the reductions so far,
 *             until rank C or the columns run out.  Reduced s zero on every non-pivot row:
 *             e = the unique solution supported on the pivot columns, d_ehat = z xor e,
 *             d_status = 0.  Otherwise d_ehat = z, d_status = 1.
 * d_x [B*N], d_pred [B*V] and d_ehat [B*V] in dtype (GNND_F32 / GNND_F64; GNND_BF16:
 * GNND_ERR_UNSUPPORTED); d_ehat holds exactly 0.0 / 1.0 and feeds gnnd_decision_errors as is;
 * d_status [B] int32.  One launch, one wave per codeword, the bit matrix in LDS: a graph whose
 * rows (C x (ceil(V/32) + 1) words, plus keys and order) exceed 64 KiB, or with C > 2048,
 * returns GNND_ERR_UNSUPPORTED with nothing launched.
 * gnnd_osd0_host is the host mirror (same definition, same bits, plain C++, no device; the
 * graph as the edge list gnnd_graph_create takes, h_* host arrays).                          */
typedef enum gnnd_osd_base { GNND_OSD_BASE_ZERO = 0, GNND_OSD_BASE_HARD = 1 } gnnd_osd_base;
int gnnd_osd0(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred, int base,
              void* d_ehat, int32_t* d_status, int64_t batch, void* stream);
int gnnd_osd0_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                   const void* h_pred, int base, void* h_ehat, int32_t* h_status, int64_t batch);

/* ---- higher-order OSD: combination sweep and exhaustive reprocessing ----------------------
 * OSD-0 returns the one solution supported on the first independent columns.  gnnd_osd starts
 * there and picks the lightest of a fixed list of further solutions ("OSD-CS" / "OSD-E" of
 * BP+OSD).  Target t, base z, keys, column order with its tie rule, pivot rule and failure rule
 * are those of gnnd_osd0, unchanged.  After its Gauss-Jordan, per codeword, with (r_i, j_i) the
 * pivot rows and columns, s the reduced residual syndrome and A the reduced matrix:
 *   failure    gnnd_osd0 would fail (an unused row keeps s = 1): d_ehat = z, d_status = 1,
 *              d_choice = 0; no candidate is tried.
 *   free       f_0 .. f_{F-1}: every non-pivot column, in the column order (descending key,
 *              ties by ascending v): the dependent columns met before rank C was reached and
 *              every column after the walk stopped.
 *   candidate  a set S of free columns: e[f] = 1 for f in S, e[j_i] = s[r_i] xor XOR_{f in S}
 *              A[r_i][f], e = 0 elsewhere.  Every candidate satisfies the syndrome.  Its cost
 *              is the Hamming weight of e: the flips relative to the base z (for
 *              GNND_OSD_BASE_ZERO the weight of the estimate itself).  An integer: the result
 *              is exact in both dtypes.
 *   methods    lambda = min(order, F)
 *              GNND_OSD_0   only the empty set; `order` is ignored (but must be >= 0): bit for
 *                           bit gnnd_osd0.
 *              GNND_OSD_CS  candidate 0 the empty set; 1 .. F the singles {f_0} .. {f_{F-1}}
 *                           (all free columns, whatever the order); then the pairs {f_a, f_b},
 *                           a < b < lambda, in lexicographic (a, b) order.  order <= 64.
 *              GNND_OSD_E   candidate m = 0 .. 2^lambda - 1 holds f_i iff bit i of m is set.
 *                           order <= 12.
 *   choice     the candidate of minimum cost, ties to the lowest candidate index: d_ehat =
 *              z xor e, d_status = 0, d_choice = that index.
 * A negative order, one above the method's limit, or an unknown method: GNND_ERR_INVALID_ARG.
 * dtypes, layouts and the LDS limits (GNND_ERR_UNSUPPORTED, nothing launched) as for gnnd_osd0;
 * d_choice [B] int32 may be NULL.  One launch on `stream`, no host sync (capturable); batch 0
 * returns GNND_OK.  gnnd_osd_host is the host mirror: same definition, same bits.             */
typedef enum gnnd_osd_method { GNND_OSD_0 = 0, GNND_OSD_CS = 1, GNND_OSD_E = 2 } gnnd_osd_method;
int gnnd_osd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred, int base,
             int method, int32_t order, void* d_ehat, int32_t* d_status, int32_t* d_choice,
             int64_t batch, void* stream);
int gnnd_osd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                  int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                  const void* h_pred, int base, int method, int32_t order, void* h_ehat,
                  int32_t* h_status, int32_t* h_choice, int64_t batch);

/* ---- min-sum BP with syndrome-converged early stop ----------------------------------------
 * Normalized / offset min-sum belief propagation on the flooding schedule (the "BP" of the usual
 * BP+OSD stacks and of hardware LDPC decoders): no transcendental in the loop, and a codeword
 * stops as soon as its hard decision satisfies the measured syndrome.  Only add, subtract, one
 * multiply, min, abs and compare touch the messages, and their order is fixed below, so d_llr,
 * d_iters and d_status are bit-reproducible in `dtype` (T = float / double).  Per codeword b,
 * edges in the single-graph order (sorted by (v, c)), E(v) / E(c) the edges at a variable / check:
 *   prior     l_v = x[b*N + v]
 *   target    t_c = (x[b*N + V + c] < 0)                      (the convention of gnnd_osd0)
 *   a = (T)alpha, b = (T)beta, each rounded to T once
 *   q_e = l_{v(e)} for every edge; then for it = 1 .. iters:
 *     check step, every edge e at check c:
 *       neg = t_c xor parity of #{ e' in E(c), e' != e : q_e' < 0 }
 *       m   = min over e' in E(c), e' != e of |q_e'|
 *       d   = round(round(a * m) - b)        two roundings in T, never a fused multiply-add
 *       mag = d > 0 ? d : +0
 *       r_e = neg ? -mag : mag
 *     variable step, every variable v:
 *       L_v = ((l_v + r_e1) + r_e2) + ...    E(v) in ascending edge order, left to right, in T
 *       q_e = L_v - r_e for e in E(v)
 *     h_v = (L_v < 0);  ok = (H^T h == t on every check);  if early_stop and ok: stop
 *   `q < 0` is false for -0.0.  "Min over the others" is literal: two edges tying for the
 *   minimum both see that minimum (the first-min / second-min / arg-min form is equivalent).
 * Outputs: d_out[b*V + v] = 1 / (1 + exp(L_v)) = P(bit = 1), the tensor gnnd_osd and
 * gnnd_decision_errors take (not part of the bit-exact contract: exp is the library's);
 * d_llr[b*V + v] = L_v of the last executed iteration; d_iters[b] = iterations executed;
 * d_status[b] = 0 if ok held after the last executed iteration, else 1 (the sense of gnnd_osd's
 * status; with early_stop = 0 all `iters` iterations run and the status describes the last).
 * d_x [B*N], d_out / d_llr [B*V] in dtype, d_iters / d_status [B] int32; d_llr, d_iters and
 * d_status may each be NULL, d_out is required.  x must be finite: a codeword holding a NaN or an
 * infinity has unspecified outputs, but does not fault and touches no other codeword's outputs.
 * iters < 1, alpha not finite or outside (0, 1], beta not finite or < 0, early_stop not 0 / 1, or
 * a NULL required pointer: GNND_ERR_INVALID_ARG, decided before any device call.  GNND_BF16, a
 * graph with a check of degree < 2, or a per-codeword LDS tile ((E + 2 V) values of T) over
 * 64 KiB: GNND_ERR_UNSUPPORTED, nothing launched.  batch 0 returns GNND_OK.  One launch on
 * `stream`, one wave per codeword, no host sync (capturable).
 * gnnd_minsum_host is the host mirror (plain C++, no device; the graph as the edge list
 * gnnd_graph_create takes): the same definition, the same bits in llr / iters / status.      */
int gnnd_minsum(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
                int32_t iters, int32_t early_stop, void* d_out, void* d_llr,
                int32_t* d_iters, int32_t* d_status, int64_t batch, void* stream);
int gnnd_minsum_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                     int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                     double alpha, double beta, int32_t iters, int32_t early_stop,
                     void* h_out, void* h_llr, int32_t* h_iters, int32_t* h_status,
                     int64_t batch);

/* ---- gated OSD and the one-call BP+OSD decoder ---------------------------------------------
 * gnnd_osd_gated is gnnd_osd on the codewords the caller's gate selects, the way every BP+OSD
 * decoder joins its two stages: a codeword whose BP hard decision already satisfies its syndrome
 * keeps that decision, only the others are reprocessed.  Per codeword b:
 *   d_gate[b] != 0  d_ehat, d_status and d_choice of b are bit for bit what gnnd_osd writes for
 *                   that codeword with the same base, method and order.  Codewords are
 *                   independent: the result does not depend on which others are gated.
 *   d_gate[b] == 0  pass-through: d_ehat[b*V + v] = h_v as exactly 0.0 / 1.0, d_status[b] = 0,
 *                   d_choice[b] = -1, with the hard decision
 *                     h_v = (d_llr[b*V + v] < 0)     if d_llr is not NULL (min-sum's own hard
 *                                                    decision: false for -0.0 and for a NaN)
 *                     h_v = (d_pred[b*V + v] > 0.5)  if d_llr is NULL (a NaN gives 0)
 *                   The syndrome of a pass-through codeword is not re-checked: the gate is the
 *                   caller's claim.  d_llr exists because pred = 1 / (1 + exp(L)) rounds to
 *                   exactly 0.5 for a tiny |L|, and (pred > 0.5) then loses a decision that
 *                   min-sum's status was computed from.
 * d_gate [B] int32 (gnnd_minsum's d_status is one); d_llr [B*V] in dtype or NULL; the other
 * arrays as for gnnd_osd, d_choice may be NULL.  d_work is the caller's scratch of at least
 * gnnd_osd_gated_workspace(batch) bytes (4 * (batch + 1): an int32 count and the int32 list of
 * gated codewords), 4-byte aligned, contents unspecified before and after; the library allocates
 * nothing.  Two launches on `stream`: a compaction that writes the ascending list of gated
 * codewords and the pass-through outputs, then gnnd_osd's kernel plan over that list, its length
 * read on the device.  No host read of the gate and no synchronisation (capturable; a replay
 * follows the gate it finds).
 * base, method, order and dtype are checked as in gnnd_osd; a NULL required pointer or work_bytes
 * below the workspace size: GNND_ERR_INVALID_ARG, decided before any device call.  The LDS and C
 * limits of gnnd_osd, or batch > 2^31 - 2: GNND_ERR_UNSUPPORTED, nothing launched.  batch 0
 * returns GNND_OK.  gnnd_osd_gated_host is the host mirror: same definition, same bits.
 *
 * gnnd_bposd is gnnd_minsum(d_x, alpha, beta, iters, early_stop -> d_pred, d_llr, d_iters,
 * d_bp_status) followed by gnnd_osd_gated(d_x, d_pred, d_llr, gate = d_bp_status, base, method,
 * order -> d_ehat, d_status, d_choice) on the same stream: three launches, no host sync.  d_pred,
 * d_llr and d_bp_status are required (they feed the second stage); d_iters and d_choice may be
 * NULL.  The outputs inherit the two contracts: d_llr, d_iters and d_bp_status are
 * bit-reproducible (gnnd_minsum), and d_ehat, d_status and d_choice are gnnd_osd_gated's
 * bit-exact function of d_x, d_pred, d_llr and the gate.  d_pred is gnnd_minsum's soft output.
 * In GNND_F64 its exponential is a fixed sequence of correctly rounded operations (k = rint(L
 * log2 e), r = L - k ln2 with a two-part ln2, a degree-13 Taylor polynomial by Horner in fused
 * multiply-adds, ldexp), which gnnd_bposd_host repeats: there d_pred, and with it d_ehat,
 * d_status and d_choice, are the same bits on the device and in the host mirror.  In GNND_F32 the
 * device uses its math library's expf: d_pred may differ from the mirror's in the last place, and
 * a codeword in which that changes the order of two nearly equal columns may get another
 * (equally valid) estimate; pass-through codewords agree bit for bit in both dtypes.
 * Guarantee: where d_bp_status[b] == 0, d_ehat of b is min-sum's own
 * hard decision (d_llr < 0) and satisfies the syndrome exactly; elsewhere it is gnnd_osd's
 * estimate, which satisfies it wherever d_status[b] == 0.
 * Every GNND_ERR_INVALID_ARG of either stage is decided before the first device call;
 * GNND_ERR_UNSUPPORTED is the union of both stages' conditions, with nothing launched; batch 0
 * returns GNND_OK.  gnnd_bposd_host is the host mirror (gnnd_minsum_host's loop with that fp64
 * exponential for the soft output, then gnnd_osd_gated_host).                                  */
int gnnd_osd_gated_workspace(int64_t batch, int64_t* h_bytes);
int gnnd_osd_gated(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                   const void* d_llr, const int32_t* d_gate, int base, int method, int32_t order,
                   void* d_ehat, int32_t* d_status, int32_t* d_choice, void* d_work,
                   int64_t work_bytes, int64_t batch, void* stream);
int gnnd_osd_gated_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                        int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                        const void* h_pred, const void* h_llr, const int32_t* h_gate, int base,
                        int method, int32_t order, void* h_ehat, int32_t* h_status,
                        int32_t* h_choice, int64_t batch);
int gnnd_bposd(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
               int32_t iters, int32_t early_stop, int base, int method, int32_t order,
               void* d_pred, void* d_llr, int32_t* d_iters, int32_t* d_bp_status, void* d_ehat,
               int32_t* d_status, int32_t* d_choice, void* d_work, int64_t work_bytes,
               int64_t batch, void* stream);
int gnnd_bposd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                    int32_t num_var, int32_t num_chk, int dtype, const void* h_x, double alpha,
                    double beta, int32_t iters, int32_t early_stop, int base, int method,
                    int32_t order, void* h_pred, void* h_llr, int32_t* h_iters,
                    int32_t* h_bp_status, void* h_ehat, int32_t* h_status, int32_t* h_choice,
                    int64_t batch);

/* ---- layered-schedule min-sum BP and the layered one-call BP+OSD decoder ---------------------
 * gnnd_minsum on the layered (serial, check-sequential) schedule: the checks are visited one
 * after another and each sees the variable posteriors the checks before it just updated, the
 * usual way to reach a decision in about half the iterations of the flooding schedule.
 * Layers.  Computed once per graph on the host, in gnnd_graph_create.  Checks are taken in
 * ascending c; layer(c) is the smallest k >= 0 such that no check c' < c with layer(c') == k
 * shares a variable with c.  The layered order is the checks sorted by (layer, c).  Two checks of
 * one layer share no variable.  gnnd_graph_layers returns the number of layers and, where
 * h_layer_of_check [C] is not NULL, layer(c); gnnd_graph_layers_host is the same rule on the edge
 * list gnnd_graph_create takes, with no device (both: a NULL graph / edge list / h_nlayers is
 * GNND_ERR_INVALID_ARG; the host form checks the edge list as gnnd_minsum_host does).
 * Loop.  Per codeword b, T = float / double; a, b, t_c, l_v, the edge order and the x / output
 * layouts exactly as in gnnd_minsum:
 *   L_v = l_v for every variable;  r_e = +0 for every edge
 *   for it = 1 .. iters:
 *     for c in the layered order:
 *       q_e = L_v(e) - r_e                for e in E(c)     (one subtraction in T)
 *       neg, m, d = round(round(a * m) - b), mag, r'_e      gnnd_minsum's check step over these
 *                                                            q_e, literally (ties, -0.0, two
 *                                                            roundings, no fused multiply-add)
 *       L_v(e) = q_e + r'_e ;  r_e = r'_e  for e in E(c)     (one addition in T)
 *     h_v = (L_v < 0);  ok = (H^T h == t on every check);  if early_stop and ok: stop
 * The checks of a layer touch disjoint L_v, so any order or parallelism inside a layer gives the
 * bits of this serial statement; the kernel relies on that.
 * Outputs, NULL rules, argument checks, non-finite behaviour, GNND_ERR_* conditions and batch 0
 * follow gnnd_minsum word for word, with one exception: the per-codeword LDS tile is (E + V)
 * values of T (no separate prior array), refused with GNND_ERR_UNSUPPORTED over 64 KiB.  d_llr,
 * d_iters and d_status are bit-reproducible in both dtypes; d_out is outside the contract in
 * GNND_F32 and uses gnnd_bposd's fixed exponential in GNND_F64.  One launch on `stream`, no host
 * sync (capturable): a codeword gets G lanes of a wave, G the power of two covering the largest
 * layer, clamped to [8, 64] (raised where 64 / G tiles would not fit in 64 KiB), and a wave holds
 * 64 / G codewords.  gnnd_minsum_layered_plan reports h_plan4 = {layers, checks in the largest
 * layer, lanes per codeword, codewords per workgroup} for `dtype` (GNND_ERR_UNSUPPORTED where
 * gnnd_minsum_layered would refuse the graph).  gnnd_minsum_layered_host is the host mirror: the
 * same definition, the same bits in llr / iters / status.
 * gnnd_bposd_layered is gnnd_bposd with gnnd_minsum_layered as its first stage: the layered
 * min-sum, then the unchanged gnnd_osd_gated, three launches on `stream`, no host sync; arguments,
 * refusals (all decided before the first launch) and guarantees as for gnnd_bposd.
 * gnnd_bposd_layered_host is its mirror; in GNND_F64 d_pred goes through the same fixed
 * exponential on both sides, so every output is the same bits on the device and in the mirror. */
int gnnd_graph_layers(const gnnd_graph* g, int32_t* h_nlayers, int32_t* h_layer_of_check);
int gnnd_graph_layers_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                           int32_t num_var, int32_t num_chk, int32_t* h_nlayers,
                           int32_t* h_layer_of_check);
int gnnd_minsum_layered(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
                        int32_t iters, int32_t early_stop, void* d_out, void* d_llr,
                        int32_t* d_iters, int32_t* d_status, int64_t batch, void* stream);
int gnnd_minsum_layered_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                             double alpha, double beta, int32_t iters, int32_t early_stop,
                             void* h_out, void* h_llr, int32_t* h_iters, int32_t* h_status,
                             int64_t batch);
int gnnd_minsum_layered_plan(const gnnd_graph* g, int dtype, int32_t* h_plan4);
int gnnd_bposd_layered(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
                       int32_t iters, int32_t early_stop, int base, int method, int32_t order,
                       void* d_pred, void* d_llr, int32_t* d_iters, int32_t* d_bp_status,
                       void* d_ehat, int32_t* d_status, int32_t* d_choice, void* d_work,
                       int64_t work_bytes, int64_t batch, void* stream);
int gnnd_bposd_layered_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                            int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                            double alpha, double beta, int32_t iters, int32_t early_stop, int base,
                            int method, int32_t order, void* h_pred, void* h_llr, int32_t* h_iters,
                            int32_t* h_bp_status, void* h_ehat, int32_t* h_status,
                            int32_t* h_choice, int64_t batch);

/* ---- relay min-sum BP: memory-strength legs that keep the lightest solution ------------------
 * Min-sum with a per-variable memory term (DMem-BP), run as a chain of "legs": each leg has its own
 * memory strengths g_v (positive, zero or negative), starts from the posteriors of the leg before,
 * and ends at its first hard decision that satisfies the syndrome; the solutions are collected and
 * the lightest is kept.  Adds, one kind of multiply, mins and compares only, in the order fixed
 * below: every output is bit-reproducible in `dtype` (T = float / double).  The graph, the edge
 * order, l_v, t_c, a, b, the check step and "`q < 0` is false for -0.0" are gnnd_minsum's.
 * Inputs beside gnnd_minsum's: d_gammas [legs*V] in dtype, one row per leg, shared by every
 * codeword; legs >= 1; iters0 >= 1 the iterations of leg 0, iters_leg >= 1 those of every later
 * leg; stop_after = S >= 1.  Per codeword:
 *   M_v = l_v;  nsol = 0;  best = none;  total = 0
 *   for k = 0 .. legs-1:                                  T_k = k == 0 ? iters0 : iters_leg
 *     g_v = gammas[k*V + v];  c_v = round(1 - g_v)        in T
 *     Lam_v(M) = (g_v == 0) ? l_v                         selected, not computed: a -0.0 prior stays
 *              : round(round(c_v * l_v) + round(g_v * M_v))   three roundings, no fused multiply-add
 *     q_e = Lam_{v(e)}(M)                                 the messages restart, M carries over
 *     for it = 1 .. T_k:
 *       total += 1
 *       check step                                        gnnd_minsum's, on q, giving r_e
 *       variable step: L_v = ((Lam_v(M) + r_e1) + r_e2) + ...   E(v) ascending, left to right
 *                      q_e = L_v - r_e;  then M_v = L_v
 *       h_v = (L_v < 0);  ok = (H^T h == t on every check)
 *       if ok: w = weight(h);  nsol += 1
 *              if best is none or w < best.w: best = (L, k, w)    strict: a tie keeps the earlier
 *              leave leg k
 *     if nsol >= S: stop
 *   weight(h): p_j = sum over v = j (mod 64), ascending v, of (h_v ? l_v : +0), starting from +0,
 *   for j = 0 .. 63; then for s = 32, 16, 8, 4, 2, 1: p_j = p_j + p_{j xor s} (all j at once);
 *   w = p_0.  The tree is part of the contract, so the device and the mirror agree bit for bit.
 * Outputs: d_ehat [B*V] in dtype, exactly 0.0 / 1.0, required; d_llr [B*V] in dtype; d_iters,
 * d_status, d_leg, d_nsol [B] int32; these five may each be NULL.  With a best solution: ehat =
 * (best.L < 0), llr = best.L, status 0, leg = best.k, nsol the number of solutions collected, iters
 * = total.  With none: ehat and llr from the last executed iteration, status 1, leg -1, nsol 0,
 * iters = iters0 + (legs - 1) * iters_leg.  No transcendental appears anywhere in the call.
 * Guarantees: where d_status[b] == 0, d_ehat of b satisfies the syndrome exactly.  With legs = 1
 * and an all-zero gammas row, d_llr, d_iters and d_status are the bits of gnnd_minsum with iters =
 * iters0 and early_stop = 1.  x and gammas must be finite: a non-finite value leaves the outputs of
 * the codewords it touches unspecified, faults nothing and touches no other codeword's outputs (no
 * index depends on data).
 * legs, iters0, iters_leg or stop_after < 1, an iteration total iters0 + (legs - 1) * iters_leg
 * above 2^31 - 1, alpha or beta outside gnnd_minsum's limits, or a NULL d_x, d_gammas or d_ehat:
 * GNND_ERR_INVALID_ARG, decided before any device call.  GNND_BF16, a graph with a check of degree
 * < 2, or a per-codeword LDS tile over 64 KiB: GNND_ERR_UNSUPPORTED, nothing launched.  The tile is
 * (E + 4 V) values of T, each array rounded up to 16 bytes: the messages, the leg's prior term
 * round(c_v * l_v), the leg's g_v, M / L, and the best L.  batch 0 returns GNND_OK.  One launch on
 * `stream`, one wave per codeword, no host sync (capturable).  Feeding the codewords relay leaves
 * unsolved to gnnd_osd_gated needs the soft pred that gnnd_osd_gated orders the columns by:
 * gnnd_relay_soft below produces it, and gnnd_relay_osd is the pairing in one call.
 * gnnd_relay_host is the host mirror (plain C++, no device; the graph as the edge list
 * gnnd_graph_create takes, checked as gnnd_minsum_host checks it): the same definition, the same
 * bits in every output.                                                                        */
int gnnd_relay(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
               int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after, double alpha,
               double beta, void* d_ehat, void* d_llr, int32_t* d_iters, int32_t* d_status,
               int32_t* d_leg, int32_t* d_nsol, int64_t batch, void* stream);
int gnnd_relay_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                    int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                    const void* h_gammas, int32_t legs, int32_t iters0, int32_t iters_leg,
                    int32_t stop_after, double alpha, double beta, void* h_ehat, void* h_llr,
                    int32_t* h_iters, int32_t* h_status, int32_t* h_leg, int32_t* h_nsol,
                    int64_t batch);

/* ---- relay with a soft output, and the one-call relay+OSD decoder ----------------------------
 * gnnd_relay_soft is gnnd_relay, word for word: for the same arguments d_ehat, d_llr, d_iters,
 * d_status, d_leg and d_nsol are the bits gnnd_relay writes.  It adds a soft LLR Z_v per variable,
 * the one thing gnnd_osd_gated needs from a BP stage, chosen by `soft` for the codewords relay
 * could not solve: the posteriors of the last iteration (GNND_RELAY_SOFT_LAST, what gnnd_bposd
 * uses), or their mean over every iteration of every leg (GNND_RELAY_SOFT_MEAN: a chain of legs
 * with disordered memory strengths oscillates, and the mean remembers where).  Per codeword, in T:
 *   accumulator (MEAN only)   A_v = +0 before leg 0;  after the variable step of every executed
 *                             iteration of every leg: A_v = A_v + L_v        (one addition in T)
 *   scale                     inv = (T)(1.0 / (double)(iters0 + (legs - 1) * iters_leg)), computed
 *                             once on the host; the device performs no division for it
 *   status 0 (both modes)     Z_v = best.L_v, the value written to d_llr
 *   status 1, LAST            Z_v = L_v of the last executed iteration, which is d_llr
 *   status 1, MEAN            Z_v = round(A_v * inv)                         (one multiply in T);
 *                             for such a codeword the executed iteration count is exactly the
 *                             denominator of inv
 * Outputs beside gnnd_relay's: d_soft [B*V] in dtype = Z_v, may be NULL; d_pred [B*V] in dtype =
 * 1 / (1 + exp(Z_v)), required.  In GNND_F64 the exponential is gnnd_bposd's fixed sequence, which
 * the mirror repeats.  d_soft is bit-reproducible in both dtypes; d_pred is bit-reproducible in
 * GNND_F64 and outside the contract in GNND_F32 (the device's expf), exactly as for gnnd_minsum.
 * `soft` outside the enum, or a NULL d_pred: GNND_ERR_INVALID_ARG, decided before any device call.
 * Every other check, refusal, the non-finite rule and the batch-0 rule follow gnnd_relay.  One
 * launch, one wave per codeword, capturable.  The LDS tile is gnnd_relay's (E + 4 V) values for
 * LAST and (E + 5 V) for MEAN (the accumulator), each array rounded up to 16 bytes; over 64 KiB:
 * GNND_ERR_UNSUPPORTED, nothing launched.
 *
 * gnnd_relay_osd is gnnd_relay_soft(... soft -> d_pred, no d_soft, d_ehat, d_llr, d_iters,
 * d_relay_status, d_leg, d_nsol) followed by the unchanged gnnd_osd_gated(d_x, d_pred, d_llr, gate
 * = d_relay_status, base, method, order -> d_ehat, d_status, d_choice) on the same stream: three
 * launches, no host sync.  d_pred, d_llr, d_relay_status, d_ehat, d_status and d_work (as for
 * gnnd_osd_gated) are required; d_iters, d_leg, d_nsol and d_choice may be NULL.
 * Guarantee: where d_relay_status[b] == 0, d_ehat of b is relay's own kept solution (d_llr < 0),
 * which satisfies the syndrome exactly, and d_choice[b] = -1; elsewhere d_ehat of b is gnnd_osd's
 * estimate, which satisfies it wherever d_status[b] == 0.  With legs = 1, an all-zero gammas row
 * and LAST, every shared output is the bits of gnnd_bposd with iters = iters0 and early_stop = 1.
 * Every GNND_ERR_INVALID_ARG of either stage is decided before the first device call;
 * GNND_ERR_UNSUPPORTED is the union of both stages' conditions, with nothing launched; batch 0
 * returns GNND_OK.
 * gnnd_relay_soft_host and gnnd_relay_osd_host are the host mirrors (the graph as the edge list
 * gnnd_relay_host takes): the same accumulation order, the same inv, the same fixed fp64
 * exponential, then gnnd_osd_gated_host.  In GNND_F64 every output of both is the device's bits;
 * in GNND_F32 everything but d_pred is, and with it the estimates of the gated codewords under
 * gnnd_bposd's caveat (pass-through codewords agree bit for bit).                              */
typedef enum gnnd_relay_soft_mode {
    GNND_RELAY_SOFT_LAST = 0, GNND_RELAY_SOFT_MEAN = 1
} gnnd_relay_soft_mode;
int gnnd_relay_soft(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                    int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                    double alpha, double beta, int soft, void* d_pred, void* d_soft, void* d_ehat,
                    void* d_llr, int32_t* d_iters, int32_t* d_status, int32_t* d_leg,
                    int32_t* d_nsol, int64_t batch, void* stream);
int gnnd_relay_soft_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                         int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                         const void* h_gammas, int32_t legs, int32_t iters0, int32_t iters_leg,
                         int32_t stop_after, double alpha, double beta, int soft, void* h_pred,
                         void* h_soft, void* h_ehat, void* h_llr, int32_t* h_iters,
                         int32_t* h_status, int32_t* h_leg, int32_t* h_nsol, int64_t batch);
int gnnd_relay_osd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                   int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                   double alpha, double beta, int soft, int base, int method, int32_t order,
                   void* d_pred, void* d_llr, int32_t* d_iters, int32_t* d_relay_status,
                   int32_t* d_leg, int32_t* d_nsol, void* d_ehat, int32_t* d_status,
                   int32_t* d_choice, void* d_work, int64_t work_bytes, int64_t batch,
                   void* stream);
int gnnd_relay_osd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                        int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                        const void* h_gammas, int32_t legs, int32_t iters0, int32_t iters_leg,
                        int32_t stop_after, double alpha, double beta, int soft, int base,
                        int method, int32_t order, void* h_pred, void* h_llr, int32_t* h_iters,
                        int32_t* h_relay_status, int32_t* h_leg, int32_t* h_nsol, void* h_ehat,
                        int32_t* h_status, int32_t* h_choice, int64_t batch);

/* ---- min-sum BP with guided decimation: freeze bits between BP rounds -------------------------
 * BP guided decimation (BPGD), the elimination-free cure for the degeneracy that traps BP on
 * quantum codes: a few min-sum iterations, then the prior of one (or a few) variables is frozen at
 * a large LLR of the sign BP currently gives it, and BP goes on from the same messages.  `pick`
 * chooses which variables: GNND_BPGD_LEAST the least reliable ones (smallest |L_v|: it breaks the
 * symmetric ties of a degenerate code), GNND_BPGD_MOST the most reliable ones (largest |L_v|: the
 * published rule for hypergraph-product codes).  Adds, one kind of multiply, mins and compares
 * only, in the order fixed below.  The graph, the edge order, l_v, t_c, a, b, the check step, the
 * variable-sum order and "`q < 0` is false for -0.0" are gnnd_minsum's, unchanged; T = float /
 * double.  iters0 >= 1 the iterations before the first decimation, iters_round >= 1 those after
 * every decimation, rounds >= 0 the decimation rounds, per_round >= 1 the variables frozen per
 * round.  Per codeword:
 *   p_v = l_v;  dec_v = 0;  ndec = 0;  total = 0;  q_e = p_v(e);  c = (T)clamp, rounded once
 *   for r = 0 .. rounds:                                  T_r = r == 0 ? iters0 : iters_round
 *     for it = 1 .. T_r:
 *       total += 1
 *       check step                                        gnnd_minsum's, on q, giving r_e
 *       variable step: L_v = ((p_v + r_e1) + r_e2) + ...  E(v) ascending, left to right
 *                      q_e = L_v - r_e
 *       h_v = (L_v < 0);  ok = (H^T h == t on every check);  if ok: status 0, stop
 *     if r == rounds or ndec == V: status 1, stop
 *     repeat min(per_round, V - ndec) times, every pick reading the same L (this round's last):
 *       v* = among dec_v == 0 the variable of minimum (LEAST) / maximum (MOST) |L_v|, ties to the
 *            lowest v: an ascending scan that starts at the first undecimated variable and moves
 *            on a strict compare only
 *       p_v* = (L_v* < 0) ? -c : c;  dec_v* = 1;  ndec += 1
 *     (the messages are not restarted: only p changes, and the next variable step sees it)
 * Outputs: d_ehat [B*V] in dtype, exactly 0.0 / 1.0 = (L_v < 0) of the last executed iteration,
 * required; d_llr [B*V] in dtype = that L; d_pred [B*V] in dtype = 1 / (1 + exp(L_v)), in GNND_F64
 * through gnnd_bposd's fixed exponential (the mirror's bits), in GNND_F32 outside the contract (the
 * device's expf), as elsewhere; d_iters [B] = total, d_status [B], d_ndec [B] = ndec, int32.  Every
 * output except d_ehat may be NULL.  d_pred, d_status and d_llr are what gnnd_osd_gated takes, so
 * the codewords left at status 1 can be handed on as they are.
 * Guarantees: where d_status[b] == 0, d_ehat of b satisfies the syndrome exactly.  With rounds ==
 * 0, d_llr, d_iters and d_status are the bits of gnnd_minsum with iters = iters0 and early_stop =
 * 1.  d_ehat, d_llr, d_iters, d_status and d_ndec are bit-reproducible in both dtypes and equal to
 * the host mirror's.  x must be finite: a non-finite value leaves the outputs of its codeword
 * unspecified, faults nothing and touches no other codeword's outputs.  The pick is the one index
 * in the call that depends on data; by its definition v* is an in-range undecimated variable
 * whatever the data holds (a NaN never wins a strict compare, and the scan starts at a variable,
 * not at a sentinel).
 * iters0 < 1, iters_round < 1, rounds < 0, per_round < 1, an iteration total iters0 + rounds *
 * iters_round above 2^31 - 1, `pick` outside the enum, clamp not finite or <= 0 (or, in GNND_F32,
 * above the largest float: c itself must be finite), alpha or beta outside gnnd_minsum's limits,
 * or a NULL d_x or d_ehat: GNND_ERR_INVALID_ARG, decided before any device call.  GNND_BF16, a
 * graph with a check of degree < 2, or a per-codeword LDS tile over 64 KiB: GNND_ERR_UNSUPPORTED,
 * nothing launched.  The tile is (E + 2 V) values of T and V int32, each array rounded up to 16
 * bytes: the messages, the mutable prior p, L, and the decimated flags.  batch 0 returns GNND_OK.
 * One launch on `stream`, one wave per codeword, no host sync (capturable).
 * gnnd_bpgd_host is the host mirror (plain C++, no device; the graph as the edge list
 * gnnd_graph_create takes, checked as gnnd_minsum_host checks it): the same definition, the same
 * bits in every output of the contract, and in GNND_F64 in h_pred too.                         */
typedef enum gnnd_bpgd_pick { GNND_BPGD_LEAST = 0, GNND_BPGD_MOST = 1 } gnnd_bpgd_pick;
int gnnd_bpgd(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
              int32_t iters0, int32_t iters_round, int32_t rounds, int32_t per_round, int pick,
              double clamp, void* d_ehat, void* d_llr, void* d_pred, int32_t* d_iters,
              int32_t* d_status, int32_t* d_ndec, int64_t batch, void* stream);
int gnnd_bpgd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t num_var,
                   int32_t num_chk, int dtype, const void* h_x, double alpha, double beta,
                   int32_t iters0, int32_t iters_round, int32_t rounds, int32_t per_round, int pick,
                   double clamp, void* h_ehat, void* h_llr, void* h_pred, int32_t* h_iters,
                   int32_t* h_status, int32_t* h_ndec, int64_t batch);

/* ---- union-find decoding of a matchable code: grow, merge, peel --------------------------------
 * The decoder one reaches for first on a toric or surface code: clusters grow around the defects
 * by half-edges, merge when they meet, and stop once each holds an even number of defects; a
 * spanning forest of every cluster is then peeled from the leaves.  Integers only, no iteration
 * count or damping, no elimination; the priors in x are not read.
 * Graphs.  The Tanner graph must be matchable: every variable of degree 1 or 2 (toric_code(L) is;
 * one plaquette of each half is left out of H, so a few variables have degree 1).  Its decoding
 * graph, built once per graph on the host and kept with it:
 *   vertices  0 .. C-1 the checks; then one virtual vertex for every connected component of the
 *             Tanner graph that holds a degree-1 variable, the components taken in ascending order
 *             of their lowest check and numbered C, C+1, ..; K of them, N = C + K.  A virtual
 *             vertex stands for the check left out of H: its syndrome bit is whatever makes its
 *             component's parity even.
 *   edges     variable v is the edge (a_v, b_v), a_v < b_v: its two checks, or its check and its
 *             component's virtual vertex.  Parallel edges are legal; self-loops cannot occur.
 * gnnd_graph_matching returns N in *h_nvert and, where h_endpoints [2 V] is not NULL, a_v at 2 v
 * and b_v at 2 v + 1; gnnd_graph_matching_host is the same rule on the edge list gnnd_graph_create
 * takes.  A graph that is not matchable: GNND_ERR_UNSUPPORTED from both.
 * Per codeword b:
 *   t_c = (x[b (V + C) + V + c] < 0)                      gnnd_osd0's convention; a NaN gives 0
 *   defect[u] = t_u for u < C; for a virtual u the XOR of t_c over its component's checks
 *   grow[v] = 0;  label[u] = u;  rounds = 0;  status = 0
 *   growth round:
 *     odd[l] = XOR of defect[u] over the vertices with label[u] == l
 *     if no l is odd: growth ends
 *     every edge v: grow[v] = min(2, grow[v] + odd[label[a_v]] + odd[label[b_v]]), all edges from
 *       the same labels: one half-edge from each end that lies in an odd cluster
 *     if no edge changed: status = 1, growth ends (see below); the round is not counted
 *     rounds += 1
 *     labels: those of the connected components over the edges with grow == 2, a component's
 *       label its highest vertex index (the fixed point of label[u] <- max over full edges)
 *   forest: over the full edges, depth[u] = the BFS distance from u's label vertex, the root (the
 *     virtual vertex whenever the cluster holds one: virtual indices are the highest); the parent
 *     edge of a non-root u = the lowest-numbered full edge (u, w) with depth[w] == depth[u] - 1
 *   peel: ehat[v] = 1 exactly where v is the parent edge of some u and the defects over u's
 *     subtree XOR to 1; every other edge 0
 * Termination.  Every component with a virtual vertex has even parity by construction, so an odd
 * cluster is never a whole component and always has an edge that is not yet full: some edge grows
 * in every round and growth ends within 2 V rounds, with no round limit.  A component WITHOUT a
 * virtual vertex whose syndrome has odd parity has no e with H^T e = t at all; there an odd
 * cluster ends up as the whole component, a round changes nothing, and the decoder stops with
 * status 1 (ehat then satisfies every check but that cluster's root).  Nothing else gives status 1.
 * Outputs: d_ehat [B*V] in dtype, exactly 0.0 / 1.0, required (it feeds gnnd_decision_errors as
 * is); d_rounds [B] int32 the growth rounds executed; d_status [B] int32, 0 for a decoded
 * codeword, so the result drops into the places that take a status; d_nfull [B] int32 the number
 * of full edges when growth ended.  The last three may be NULL.
 * Gate: d_gate [B] int32 may be NULL.  With a gate, a codeword whose gate is 0 is skipped and none
 * of its outputs is written: after gnnd_bpgd, gnnd_relay or gnnd_minsum, their d_status as the gate
 * and their d_ehat (or hard decision) as d_ehat overwrites exactly the unsolved rows.
 * Guarantees: where d_status[b] == 0, and so for every codeword of a graph whose components all
 * have a virtual vertex, d_ehat of b satisfies the syndrome exactly, for any x: only the signs of
 * the check rows are read, a NaN compares false and faults nothing.  All outputs are
 * bit-reproducible and equal to the host mirror's, in GNND_F32 and GNND_F64 (nothing but the input
 * and output formats depends on the dtype).  A codeword with zero syndrome returns zero, rounds 0,
 * nfull 0.
 * Kernel: one launch on `stream`, one wave per codeword, no host sync (capturable).  The wave's
 * LDS tile is (V + 4 N) int32, each of the five arrays rounded up to 16 bytes: grow [V], label [N],
 * defect / subtree parity [N], odd / depth [N], parent edge [N].  No data-dependent index leaves
 * its array: a label starts as its own vertex and is only ever replaced by another vertex's label;
 * a depth is 0 at a root, else one more than a neighbour's, and is only compared; a parent is the
 * index of an edge the parent pass visited and is read only for a vertex of depth >= 1, which has
 * such an edge.  The debug build checks each of them.
 * A NULL g, d_x or d_ehat or a dtype outside the enum: GNND_ERR_INVALID_ARG.  GNND_BF16, a graph
 * that is not matchable (a variable of degree 0 or above 2), or a per-codeword tile over 64 KiB:
 * GNND_ERR_UNSUPPORTED.  All decided before any device call, nothing launched.  batch 0 returns
 * GNND_OK.
 * gnnd_uf_host is the host mirror (plain C++, no device, no tile limit): the same definition, the
 * same refusals, the same bits in every output.                                                 */
int gnnd_graph_matching(const gnnd_graph* g, int32_t* h_nvert, int32_t* h_endpoints);
int gnnd_graph_matching_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int32_t* h_nvert,
                             int32_t* h_endpoints);
int gnnd_uf(const gnnd_graph* g, int dtype, const void* d_x, const int32_t* d_gate, void* d_ehat,
            int32_t* d_rounds, int32_t* d_status, int32_t* d_nfull, int64_t batch, void* stream);
int gnnd_uf_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t num_var,
                 int32_t num_chk, int dtype, const void* h_x, const int32_t* h_gate, void* h_ehat,
                 int32_t* h_rounds, int32_t* h_status, int32_t* h_nfull, int64_t batch);

/* ---- weighted union-find and the one-call belief-find decoder --------------------------------
 * gnnd_ufw is gnnd_uf with an edge's length its quantised reliability instead of 1 for every edge:
 * clusters grow fast through bits believed flipped and slowly through reliable ones.  Fed the
 * posteriors of a BP decoder it is "belief-find".  The graphs, the decoding graph
 * (gnnd_graph_matching) and the refusals are gnnd_uf's.  Per codeword b, T = float / double:
 *   reliability  r_v = d_llr[b*V + v] if d_llr is not NULL, else the prior x[b*N + v]; the sign
 *                convention is min-sum's, positive = the bit is believed 0
 *   weight       s = (T)scale, rounded once;  m = r_v * s, one multiply in T
 *                w_v = wmax          if m >= (T)(wmax - 1)
 *                w_v = 1 + (int)m    else if m > 0         (truncation; 1 <= w_v <= wmax - 1)
 *                w_v = 1             otherwise
 *                a NaN, a negative or zero reliability and inf * 0 all compare false and give 1;
 *                +inf with scale > 0 gives wmax
 *                len_v = 2 w_v half-units
 *   set-up       defect[u], the virtual vertices, label[u] = u as in gnnd_uf;  grow[v] = 0;
 *                rounds = events = status = 0
 *   growth event:
 *     odd[l] as in gnnd_uf; if no l is odd: growth ends
 *     rate_v = odd[label[a_v]] + odd[label[b_v]]
 *     edge v is active if rate_v > 0 and grow[v] < len_v
 *     if no edge is active: status = 1, growth ends (the unsatisfiable component of gnnd_uf)
 *     d = min over the active v of ceil((len_v - grow[v]) / rate_v)
 *     every edge v: grow[v] = min(len_v, grow[v] + rate_v d), all edges from the same labels
 *     rounds += d;  events += 1
 *     labels: the fixed point of label[u] <- max over the edges with grow[v] == len_v
 *   forest, parent edges, peel: gnnd_uf's, word for word, with "full" meaning grow[v] == len_v
 * A jump of d is d unit steps (every edge grows rate_v half-units per step) between which no edge
 * fills, so no label and no parity can change between them: the definition is the unit-step one,
 * and rounds counts unit steps.  Every event fills at least one edge: events <= V, rounds <=
 * 2 wmax V, no round limit.
 * Anchor: with scale = 0 every w_v is 1, and d_ehat, d_rounds, d_status and d_nfull are bit for bit
 * gnnd_uf's; so they are with wmax = 1.
 * Outputs: d_ehat [B*V] in dtype, exactly 0.0 / 1.0, required; d_rounds, d_status, d_nfull as for
 * gnnd_uf; d_events [B] int32 the growth events.  The last four may be NULL.
 * Gate: d_gate [B] int32 may be NULL.  passthrough == 0: as gnnd_uf, a codeword whose gate is 0 is
 * skipped and none of its outputs is written.  passthrough == 1 (needs d_gate and d_llr): such a
 * codeword gets ehat_v = (d_llr[b*V + v] < 0) as exactly 0.0 / 1.0, false for -0.0 and a NaN (the
 * pass-through of gnnd_osd_gated), and status = rounds = nfull = events = 0; its syndrome is not
 * re-checked, the gate is the caller's claim.
 * Guarantees: gnnd_uf's.  Where d_status[b] == 0 of a decoded codeword, d_ehat of b satisfies the
 * syndrome exactly, for any x and any llr (a NaN or an infinity only changes a weight).  All
 * outputs are bit-reproducible and equal to the host mirror's, in GNND_F32 and GNND_F64: the
 * weight is one multiply and two compares in T, everything after it integers, each step an XOR, a
 * min, or the unique fixed point of a monotone sweep (order free).
 * Kernel: one launch on `stream`, one wave per codeword, no host sync (capturable).  The tile is
 * gnnd_uf's (V + 4 N) int32 with the length that remains, len_v - grow[v], in the edge array (full
 * is 0); the weights are computed by the wave from global memory at set-up.
 * scale not finite or < 0, wmax outside [1, 1024] (rounds stays inside int32 for V <= 65535),
 * passthrough not 0 / 1, passthrough == 1 without d_gate or d_llr, a NULL g, d_x or d_ehat, a dtype
 * outside the enum: GNND_ERR_INVALID_ARG.  GNND_BF16, a graph that is not matchable, or a tile over
 * 64 KiB: GNND_ERR_UNSUPPORTED.  All decided before any device call, nothing launched.  batch 0
 * returns GNND_OK.  gnnd_ufw_host is the host mirror (no device, no tile limit): the same
 * definition, the same refusals, the same bits in every output.
 *
 * gnnd_belief_find is gnnd_minsum(d_x, alpha, beta, iters, early_stop -> d_pred, d_llr, d_iters,
 * d_bp_status) followed by gnnd_ufw(d_x, d_llr, scale, wmax, gate = d_bp_status, passthrough = 1
 * -> d_ehat, d_rounds, d_status, d_nfull, d_events) on the same stream: two launches, no
 * workspace, no host sync (capturable).  d_pred, d_llr, d_bp_status and d_ehat are required; the
 * rest may be NULL.  Where d_bp_status[b] == 0, d_ehat of b is min-sum's own hard decision, which
 * satisfies the syndrome, and rounds = nfull = events = 0; elsewhere it is gnnd_ufw's estimate on
 * the posteriors min-sum stopped with.  On a matchable graph whose components all have a virtual
 * vertex d_ehat satisfies the syndrome for every codeword.  Every output but d_pred is
 * bit-reproducible and equal to the mirror's in both dtypes (d_pred as for gnnd_bposd: the
 * mirror's bits in GNND_F64).  Every GNND_ERR_INVALID_ARG of either stage is decided before the
 * first device call; GNND_ERR_UNSUPPORTED is the union of both stages' conditions, with nothing
 * launched; batch 0 returns GNND_OK.  gnnd_belief_find_host is the host mirror.               */
int gnnd_ufw(const gnnd_graph* g, int dtype, const void* d_x, const void* d_llr, double scale,
             int32_t wmax, const int32_t* d_gate, int32_t passthrough, void* d_ehat,
             int32_t* d_rounds, int32_t* d_status, int32_t* d_nfull, int32_t* d_events,
             int64_t batch, void* stream);
int gnnd_ufw_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t num_var,
                  int32_t num_chk, int dtype, const void* h_x, const void* h_llr, double scale,
                  int32_t wmax, const int32_t* h_gate, int32_t passthrough, void* h_ehat,
                  int32_t* h_rounds, int32_t* h_status, int32_t* h_nfull, int32_t* h_events,
                  int64_t batch);
int gnnd_belief_find(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
                     int32_t iters, int32_t early_stop, double scale, int32_t wmax, void* d_pred,
                     void* d_llr, int32_t* d_iters, int32_t* d_bp_status, void* d_ehat,
                     int32_t* d_status, int32_t* d_rounds, int32_t* d_nfull, int32_t* d_events,
                     int64_t batch, void* stream);
int gnnd_belief_find_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                          int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                          double alpha, double beta, int32_t iters, int32_t early_stop,
                          double scale, int32_t wmax, void* h_pred, void* h_llr, int32_t* h_iters,
                          int32_t* h_bp_status, void* h_ehat, int32_t* h_status,
                          int32_t* h_rounds, int32_t* h_nfull, int32_t* h_events, int64_t batch);

/* ---- localized-statistics decoding (BP+LSD): clusters solved locally --------------------------
 * gnnd_lsd grows clusters around the unsatisfied checks, as union-find does, but on any Tanner
 * graph, and solves each cluster by gnnd_osd0's elimination restricted to the cluster's own
 * columns ("LSD-0"): the elimination is as large as the error, not as the code.  Per codeword, T =
 * float / double; the inputs and conventions are gnnd_osd0's: the target t_c = (x[b*N + V + c] <
 * 0), and from p = d_pred and `base` the base vector z, the key and the column `order`, computed
 * exactly as gnnd_osd0 computes them (a NaN: key -inf, z 0; ties to the lower index).  One more
 * parameter, bits_per_step >= 0.
 *   s = t xor H^T z;  inV[v] = 0;  inC[c] = s[c];  label[c] = c;  rounds = 0
 *   if s == 0: ehat = z, status = 0, rounds = nclus = ncols = 0, done
 *   repeat
 *     rounds += 1
 *     active checks   round 1: every c with inC[c]; later: every c with inC[c] whose label is
 *                     invalid
 *     candidates      of a cluster K: the variables v with inV[v] == 0 adjacent to an active check
 *                     labelled K
 *     join            bits_per_step == 0: every candidate of every active cluster;
 *                     bits_per_step == k > 0: per active cluster its k candidates that come first
 *                     in `order` (all of them if it has fewer); the union over the clusters joins
 *     no variable joined: status = 1, ehat = z, stop            (the failure of gnnd_osd0)
 *     closure         inV[v] = 1 for the joined v; inC[c] = 1 for every check adjacent to one
 *     labels          the connected components of the subgraph induced by {v: inV[v]} and
 *                     {c: inC[c]}; label[c] = the smallest check index of c's component
 *     eliminate       gnnd_osd0's Gauss-Jordan on freshly built rows with the syndrome word s,
 *                     walking `order` but skipping every v with inV[v] == 0 (the first unused row
 *                     holding the column is the pivot)
 *     invalid labels  label[r] of every unused row r left with s_r = 1
 *     none: e[pivot column of row r] = s_r for the used rows, ehat = z xor e, status = 0, stop
 * Every round adds a variable or stops: at most V + 1 rounds.
 * Outputs: d_ehat [B*V] in dtype, exactly 0.0 / 1.0, required.  d_status, d_rounds, d_nclus (the
 * number of clusters at the end: the distinct labels over the checks of inC) and d_ncols (the
 * variables of inV at the end) are int32 [B]; each may be NULL.  Everything is integers once
 * `order` exists: all outputs are bit-reproducible and equal to the host mirror's in both dtypes.
 * Guarantees:
 *   status   d_status equals gnnd_osd0's on every input, for every bits_per_step: a cluster that
 *            cannot grow is a whole connected component of the graph whose system has no
 *            solution, and conversely.
 *   estimate where d_status[b] == 0, d_ehat of b satisfies the syndrome exactly, and is bit for bit
 *            what gnnd_osd0 returns when its column order is the final cluster variables first,
 *            in `order` order, then the others in `order` order: after the cluster columns every
 *            unused row has s = 0, so the later pivots add nothing.
 * Kernel: one launch on `stream`, one wave per codeword on a wave-private LDS tile, no host sync
 * (capturable).  The tile is gnnd_osd0's (rows, keys, order, pivots, estimate) and three int32 per
 * check (the label and two cluster slots); the inverse order and the inV flags reuse the bytes of
 * the keys.  The rows are rebuilt from the graph every round: no second copy of the matrix.
 * A NULL g, d_x, d_pred or d_ehat, a base outside the enum, a negative bits_per_step, a dtype
 * outside the enum: GNND_ERR_INVALID_ARG.  GNND_BF16, C > 2048, or a tile over 64 KiB:
 * GNND_ERR_UNSUPPORTED.  All decided before any device call, nothing launched.  batch 0 returns
 * GNND_OK.  gnnd_lsd_host is the host mirror (no device, no tile limit).
 *
 * gnnd_lsd_gated is gnnd_lsd on the codewords the caller's gate selects: semantics, pass-through
 * rule (d_llr < 0 if d_llr is not NULL, else d_pred > 0.5), workspace (gnnd_osd_gated_workspace)
 * and launch structure (the same device-side compaction, then the LSD kernel over the list, its
 * length read on the device; two launches, no host sync) are gnnd_osd_gated's.  A pass-through
 * codeword gets status = rounds = nclus = ncols = 0.  d_gate and d_work are required too; a short
 * workspace: GNND_ERR_INVALID_ARG; batch > 2^31 - 2: GNND_ERR_UNSUPPORTED.
 *
 * gnnd_bplsd is gnnd_minsum(d_x, alpha, beta, iters, early_stop -> d_pred, d_llr, d_iters,
 * d_bp_status) followed by gnnd_lsd_gated(d_x, d_pred, d_llr, gate = d_bp_status, base,
 * bits_per_step -> d_ehat, d_status, d_rounds, d_nclus, d_ncols) on the same stream: gnnd_bposd
 * argument for argument, with bits_per_step for (method, order) and the three counters for
 * d_choice.  Three launches, no host sync.  d_pred, d_llr, d_bp_status and d_ehat are required.
 * Where d_bp_status[b] == 0 every output gnnd_bposd shares is gnnd_bposd's, bit for bit; elsewhere
 * d_ehat is gnnd_lsd's estimate on min-sum's soft output (d_pred as for gnnd_bposd: the mirror's
 * bits in GNND_F64).  Every GNND_ERR_INVALID_ARG of either stage is decided before the first
 * device call; GNND_ERR_UNSUPPORTED is the union of both stages' conditions, with nothing
 * launched; batch 0 returns GNND_OK.  gnnd_lsd_gated_host and gnnd_bplsd_host are the mirrors.  */
int gnnd_lsd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred, int base,
             int32_t bits_per_step, void* d_ehat, int32_t* d_status, int32_t* d_rounds,
             int32_t* d_nclus, int32_t* d_ncols, int64_t batch, void* stream);
int gnnd_lsd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t num_var,
                  int32_t num_chk, int dtype, const void* h_x, const void* h_pred, int base,
                  int32_t bits_per_step, void* h_ehat, int32_t* h_status, int32_t* h_rounds,
                  int32_t* h_nclus, int32_t* h_ncols, int64_t batch);
int gnnd_lsd_gated(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                   const void* d_llr, const int32_t* d_gate, int base, int32_t bits_per_step,
                   void* d_ehat, int32_t* d_status, int32_t* d_rounds, int32_t* d_nclus,
                   int32_t* d_ncols, void* d_work, int64_t work_bytes, int64_t batch,
                   void* stream);
int gnnd_lsd_gated_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                        int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                        const void* h_pred, const void* h_llr, const int32_t* h_gate, int base,
                        int32_t bits_per_step, void* h_ehat, int32_t* h_status,
                        int32_t* h_rounds, int32_t* h_nclus, int32_t* h_ncols, int64_t batch);
int gnnd_bplsd(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
               int32_t iters, int32_t early_stop, int base, int32_t bits_per_step, void* d_pred,
               void* d_llr, int32_t* d_iters, int32_t* d_bp_status, void* d_ehat,
               int32_t* d_status, int32_t* d_rounds, int32_t* d_nclus, int32_t* d_ncols,
               void* d_work, int64_t work_bytes, int64_t batch, void* stream);
int gnnd_bplsd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                    int32_t num_var, int32_t num_chk, int dtype, const void* h_x, double alpha,
                    double beta, int32_t iters, int32_t early_stop, int base,
                    int32_t bits_per_step, void* h_pred, void* h_llr, int32_t* h_iters,
                    int32_t* h_bp_status, void* h_ehat, int32_t* h_status, int32_t* h_rounds,
                    int32_t* h_nclus, int32_t* h_ncols, int64_t batch);

/* Adam(torch.optim.Adam update order, amsgrad/maximize off) on one flat parameter buffer of
 * n values with its two moment buffers; *d_step is the device-resident step count (double,
 * incremented by the call), so a whole training step with the update can be captured in one
 * HIP graph.  Single-workgroup kernel (sized for the decoders' ~10^3 parameters).          */
int gnnd_adam_step(int dtype, void* d_param, const void* d_grad, void* d_exp_avg,
                   void* d_exp_avg_sq, double* d_step, int64_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, void* stream);

/* ---- input synthesis ---------------------------------------------------
 * Decoder inputs in the batch layout above, generated on the device with Philox4x32-10
 * (counter = {word, global codeword index lo/hi, stream}, key = seed): codeword b of the
 * call is global codeword offset + b, so data-parallel shards passing offset = shard start
 * draw exactly the codewords one single-device call over the global batch would.
 *   gnnd_sample_toric  quantum/error_generate.py:252-278 (gen_syn): p uniform over h_p[n_p]
 *     (n_p <= 16) per codeword, every variable flips with probability p; d_x [B*N] =
 *     {log((1-p)/p) at variable rows, (-1)^(H^T e) at check rows}, d_y [B*V] = e.
 *   gnnd_sample_awgn   classical/CGNNI.py:125-147 (Gen_Data.AWGN, get_post): codeword =
 *     the constant word codeword_bit (d_gen_cols NULL) or m G for k uniform message bits,
 *     d_gen_cols [V][ceil(k/32)] uint32 = the generator's columns as bit masks; BPSK
 *     1 - 2c, sigma^2 = 10^(-SNR/10) with SNR = h_snr_db[(offset + b) % n_snr] (n_snr <= 16);
 *     d_x [B*N] = {2 y' / sigma^2 at variable rows, 0 at check rows}, d_y [B*V] = c.
 * gnnd_philox4x32_10 is the host mirror of the generator (known-answer tests).            */
int gnnd_sample_toric(const gnnd_graph* g, int dtype, const double* h_p, int32_t n_p,
                      uint64_t seed, int64_t offset, void* d_x, void* d_y, int64_t batch,
                      void* stream);
int gnnd_sample_awgn(const gnnd_graph* g, int dtype, const double* h_snr_db, int32_t n_snr,
                     const uint32_t* d_gen_cols, int32_t k, int32_t codeword_bit, uint64_t seed,
                     int64_t offset, void* d_x, void* d_y, int64_t batch, void* stream);
void gnnd_philox4x32_10(const uint32_t* h_ctr4, const uint32_t* h_key2, uint32_t* h_out4);

/* ---- debug build (make debug -> libgnnd_debug.so, -DGNND_DEBUG) ----------------------------
 * The kernels check the table-derived indices they otherwise trust and record violations
 * as bits (0 LDS position, 1 variable id, 2 slot, 3 node, 4 grid) instead of faulting;
 * gnnd_debug_flags synchronises the device and returns (and clears) their OR.  In release
 * builds gnnd_debug_enabled() is 0 and the flags are always 0.                             */
int gnnd_debug_enabled(void);
int gnnd_debug_flags(uint32_t* h_flags);

/* ---- misc ----------------------------------------------------------------------------- */
const char* gnnd_status_string(int status);
int gnnd_last_hip_error(void);          /* hipError_t of the last GNND_ERR_HIP, per thread */
int gnnd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GNND_H */
