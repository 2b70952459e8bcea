/*
 * relgnn_sparse_features.h — C ABI of librelgnn.so, sparse node features (the citation task's opt-in
 * `sparse_node_features` mode): a CSR matrix times a dense row table, and the same kernel over the transposed
 * structure as the weight gradient.
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * Replaces: the unnamed Keras Dense in front of the first GNN layer, models/sparse_graph_model.py:165-170 (reference
 *           file:line, relative to the reference root), for features that are stored sparse:
 *               cur_node_representations = tf.keras.layers.Dense(hidden_size, use_bias=False, activation=act)(features)
 *
 * Forward (y == NULL):
 *     out[r, :] = act( sum_j val[j] * table[col[j], :] ),   j ascending over [rowptr[r], rowptr[r + 1])
 *   `act` is a RELGNN_ACT_* id (the activation table of the library); an empty row gives act(0).
 * Gradient (y != NULL): every gathered row is first multiplied element-wise by act'(.) written in terms of the
 *   forward's output (the five activations whose derivative the output determines, or RELGNN_ACT_LINEAR):
 *     out[r, :] = sum_j val[j] * ( table[col[j], :] * dact_from_output(act, y[col[j], :]) )
 *   Run over the TRANSPOSED structure with table = dOut and y = the forward's output this is the weight gradient
 *     dW[f, :] = sum_v X[v, f] * dOut[v, :] * act'(y[v, :])
 *   in one launch.  RELGNN_ACT_GELU with y is RELGNN_EINVAL (its derivative needs the pre-activation).  There is no
 *   gradient towards val: the features are data.
 *
 * Arithmetic: float32; product and add are rounded separately (no fma), the factors of a term in the order written above.
 *
 * Summation order — a function of the row's length len = rowptr[r + 1] - rowptr[r] alone, the same bits on every run and
 * on any stream, no atomics:
 *   len <= 128 (relgnn_csr_project_split_above()): one wave adds the terms to 0 in ascending j.
 *   len  > 128: the row is cut into slabs of 512 entries (relgnn_csr_project_slab()), slab s holding entries
 *               [512 s, min(len, 512 s + 512)).  A workgroup of four waves owns a slab: wave w adds the slab's entries
 *               [128 w, 128 w + 128) to 0 in ascending j (an empty range leaves +0), and the slab's sum is
 *               ((p0 + p1) + p2) + p3.  A row of one slab is finished there.  A row of several slabs leaves each
 *               slab's sum in the workspace, and a second pass adds them in ascending s: (((s0 + s1) + s2) + ...).
 *   `slabs` and `combos` state this plan for the kernels, built by the caller from rowptr (tasks/sparse_features.py):
 *     slabs  int32 [num_slabs][4] = {row, first entry, one past the last entry, dest}: dest < 0: the slab is the whole row
 *            and is written (with the activation) to out[row]; dest >= 0: the slab's sum goes to row `dest` of ws.
 *     combos int32 [num_combos][3] = {row, first ws row, number of ws rows}: the rows of several slabs.
 *   With slabs == NULL (num_slabs == 0) every row is summed by one wave in ascending j whatever its length.
 *   Tails of the unrolled loop gather an entry of the same batch again under a scale of +0.  (A row whose own terms are
 *   non-finite may therefore come out NaN where a plain sequential sum gives an infinity.)
 *
 * A column that is not stored contributes NOTHING, even against a non-finite table row — the dense product gives
 * 0 * inf = NaN there.
 *
 * Shapes: float32 val / table / y / out / ws, int32 rowptr / col, nnz < 2^31 - 1 (RELGNN_EINVAL otherwise: rowptr is
 *   32 bits wide); n a multiple of 4 in 4 .. 1024 (relgnn_csr_project_supported; RELGNN_EUNSUPPORTED otherwise);
 *   table, y, out and ws 16-byte aligned with leading dimensions (in floats) that are multiples of 4 and >= n; ws holds
 *   ws_rows rows of n floats, at least as many as the slabs name.
 * The kernels TRUST the structure (0 <= col < table_rows, monotone rowptr, slabs inside their rows): the container
 *   validates it once on the host when it is built.  A kernel fault is never the error path.
 */
#ifndef RELGNN_SPARSE_FEATURES_H_
#define RELGNN_SPARSE_FEATURES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if rows of n floats are taken (n % 4 == 0, 4 <= n <= 1024), else 0 */
int relgnn_csr_project_supported(int32_t n);
/* rows longer than this are split over the waves of a workgroup (128) */
int64_t relgnn_csr_project_split_above(void);
/* entries per slab of a split row (512) */
int64_t relgnn_csr_project_slab(void);

int relgnn_csr_project_f32(int32_t act, const int32_t* rowptr, int64_t num_rows, const int32_t* col, const float* val,
                           int64_t nnz, const float* table, int64_t table_rows, int64_t ld_table, const float* y,
                           int64_t ld_y, int32_t n, const int32_t* slabs, int64_t num_slabs, const int32_t* combos,
                           int64_t num_combos, float* ws, int64_t ws_rows, float* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SPARSE_FEATURES_H_ */
