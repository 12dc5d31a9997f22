/*
 * eps_abi.h -- C ABI of libeps_hip.so, the MI355X (gfx950) edge-scoring engine.
 *
 * This is the drop-in boundary for the Filter-and-Rank hot path of CUAI/Edge-Proposal-Sets.
 * The reference has no FFI of its own for this path: the work is done by third-party
 * kernels (SciPy sparsetools, torch_sparse, cuBLAS) behind plain Python call sites.  Each
 * entry point below names the reference call site(s) (file:line under /root/reference)
 * whose arithmetic it replaces.  The Python host (edge-proposal-sets_amd/) binds these
 * with ctypes and keeps the reference's own signatures on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (the caller keeps the
 *     buffer alive until the stream has been synchronised); nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all
 *     calls are asynchronous on it and re-entrant; no global mutable state;
 *   - return value: EPS_OK (0) or a negative EPS_E* code; the message for the calling
 *     thread's last failure is returned by eps_last_error();
 *   - CSR graphs: rowptr int64[N+1], col int32[nnz] strictly ascending inside a row
 *     (coalesced), val float32[nnz] or NULL (NULL == every stored value is 1.0f).
 */
#ifndef EPS_ABI_H
#define EPS_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPS_ABI_VERSION 7   /* 7: the tail of the filter step with device-side sizes -- eps_score_hist / _pick_compact, eps_radix_sort_by_u / _rows, eps_rescore_runs_dev; eps_scan_screen takes a column pack, eps_scan_column_pack, eps_expand_unit_list, eps_reverse_positions_sorted (r06); 6: skipped heads -- eps_scan_heads / _hub_rows / _refine; eps_scan_window_paths / _plan / _screen take a head table (r05); 2: eps_col_sums / eps_node_weights_f64 signatures (r02); 3: 64-bit survivor count, eps_scan_* (r03); 4: eps_scan_screen takes ssum / smax; 5: eps_select_compact, eps_scan_screen marks unused slots itself (r04) */

#define EPS_OK 0
#define EPS_EINVAL (-1)   /* bad argument (null pointer, negative size, unsupported shape) */
#define EPS_ELAUNCH (-2)  /* HIP launch / runtime error */
#define EPS_ENODEV (-3)   /* no usable gfx950 device */

/* node-weight modes for eps_node_weights */
#define EPS_W_AA 0 /* 1/log(colsum), inf -> 0   (adamic_utils.py:15-16)     */
#define EPS_W_RA 1 /* 1/colsum,      inf -> 0   (train_and_eval.py:203-204) */

int eps_version(void);
const char *eps_last_error(void);

/* eps_warm_up: load every code object of the library now (one empty kernel per translation unit on a private stream, waited
 * for) instead of at the first use of each -- a fresh process pays 10-30 ms per larger unit, and filter.py is one process per
 * graph (submit_job.py:20-21).  Thread-safe; meant for a background thread at start-up.  Blocking. */
int eps_warm_up(void);

/* Number of compute units / name of the current device (host query; for launch sizing
 * reports in bench.py).  name may be NULL. */
int eps_device_info(int *n_cu, char *name, int name_len);

/* ---- K2: per-node weight table ------------------------------------------------------
 * Replaces `A.sum(0)`, `1/np.log(.)`, inf->0 (adamic_utils.py:15-16) and `1/A.sum(axis=0)`,
 * inf->0 (train_and_eval.py:203-204).
 * eps_col_sums: colsum[c] = sum_r A[r,c], accumulated in FLOAT64 (exact, hence order-independent, for integer-valued
 *               A up to 2^53): colsum_f64 (n_cols doubles, cleared here) receives the sums, colsum_f32 (optional) the
 *               same sums rounded once to float32 -- what SciPy's float32 `A.sum(0)` holds for such A.
 * eps_node_weights: w[i] = mode==AA ? 1/logf(colsum[i]) : 1/colsum[i]; +-inf -> 0   (float32 sums, float32 math).
 * eps_node_weights_f64: the same in float64 from the float64 sums: filter.py:130-141, where A is int64 and the
 *               reference's math is float64. */
int eps_col_sums(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                 int64_t n_cols, double *colsum_f64, float *colsum_f32, void *stream);
int eps_node_weights(const float *colsum, int64_t n, int mode, float *w, void *stream);
int eps_node_weights_f64(const double *colsum, int64_t n, int mode, double *w, void *stream);

/* ---- K1/K3: pair scores by CSR neighbour-list intersection ------------------------------
 * Replaces `np.sum(A[src].multiply(A_[dst]), 1)` (adamic_utils.py:22, train_and_eval.py:212)
 * and `adj[e0] (.) adj[e1]` + sparse row-sum (models.py:536-542).  For each pair p:
 *   count[p] = |N(u) ^ N(v)|                                   (int32, exact)
 *   cn[p]    = sum_w A[u,w] * A[v,w]                           (float32; == count if val NULL)
 *   wsum[p]  = sum_w A[u,w] * (A[v,w] * node_w[w])             (float32; AA / RA)
 * Any of the three outputs may be NULL (skipped); wsum needs node_w != NULL.
 * u, v: int32[n_pairs] node ids in [0, n_nodes).  One wavefront scores one pair at a time. */
int eps_pair_scores(const int64_t *rowptr, const int32_t *col, const float *val,
                    const float *node_w, int64_t n_nodes, const int32_t *u, const int32_t *v,
                    int64_t n_pairs, int32_t *count, float *cn, float *wsum, void *stream);

/* float64 accumulate with float64 node weights; wsum is float64 (filter.py:141 RA path). */
int eps_pair_scores_f64(const int64_t *rowptr, const int32_t *col, const float *val,
                        const double *node_w, int64_t n_nodes, const int32_t *u,
                        const int32_t *v, int64_t n_pairs, int32_t *count, double *wsum,
                        void *stream);

/* Column-run variant of the two calls above, same arguments and results, for pair lists in the
 * reference's candidate order (filter.py:96-109: column-major, long runs of equal v): the
 * neighbourhood of the run's v is kept as an LDS bitmap and every pair costs one read of row u.
 * Correct for ANY list (pairs off the chunk's run take an in-place search) but only fast when v
 * has runs of hundreds of pairs or more; the Python host picks it from the run statistics. */
int eps_pair_scores_grouped(const int64_t *rowptr, const int32_t *col, const float *val,
                            const float *node_w, int64_t n_nodes, const int32_t *u,
                            const int32_t *v, int64_t n_pairs, int32_t *count, float *cn,
                            float *wsum, void *stream);
int eps_pair_scores_grouped_f64(const int64_t *rowptr, const int32_t *col, const float *val,
                                const double *node_w, int64_t n_nodes, const int32_t *u,
                                const int32_t *v, int64_t n_pairs, int32_t *count, double *wsum,
                                void *stream);

/* ---- K7 (+K1): fused candidate generation and scoring of the filter stage ------------------
 * Replaces filter.py:96-109 (`A2 = adj_t @ adj_t`, remove diagonal, zero known edges, nonzeros in
 * column-major order) together with the heuristic scoring that follows it (adamic_utils.py:13-25,
 * train_and_eval.py:195-216, models.py:536-542): one expansion of the 2-hop paths of a column
 * yields every candidate of the column with its common-neighbour count and
 * sum_w A[u,w]*(A[v,w]*node_w[w]).  The adjacency must be symmetric (rank.py:33).  Id spaces of
 * up to eps_expand_max_nodes() ids fit the LDS bitmap at once; wider ones are expanded in id windows
 * of that size (each window walks only the row segments inside it), same outputs, same order.
 *   col_order (both calls; may be NULL): a permutation of [0, v_hi - v_lo) -- the order in which the
 *                     columns v_lo + col_order[i] are handed to the workgroups.  Results do not
 *                     depend on it; heaviest-first shortens the tail of a launch.
 *   eps_expand_count: cand_count[v - v_lo] = number of 2-hop non-edges (u, v), v in [v_lo, v_hi).
 *   eps_expand_fill : colptr = exclusive prefix of cand_count (int64[n_cols+1], device); writes
 *                     cand_u (ascending inside a column == the reference's order), cand_v (column
 *                     id per candidate; optional) and, each optional, the common-neighbour count
 *                     cn (int32) and the weighted sum score (float32); neither needs zeroing.
 *                     cn / score need `workspace` (device, 8-byte aligned, contents arbitrary):
 *                     eps_expand_workspace_bytes(P) bytes, P >= the largest number of two-hop
 *                     paths sum_{w in N(v)} deg(w) of any column in the range.  The paths of a
 *                     column are binned there by candidate-rank tile, then summed tile by tile in
 *                     LDS in 2^-40 fixed point: integer addition makes the sums independent of the
 *                     arrival order (P = 0 without cn / score).  colptr may also be an UPPER-BOUND
 *                     layout -- any non-decreasing int64[n_cols+1] whose segments are at least as
 *                     long as the columns' candidate counts, e.g. the prefix of the two-hop path
 *                     counts, which needs no eps_expand_count pass: cand_count (optional) then
 *                     receives the real count per column and the rest of each segment is padded
 *                     with cand_u = -1, score = -inf, cn = 0, so the arrays stay in candidate
 *                     order.  After the launch the first 4 bytes of the workspace are 0, or
 *                     non-zero if P (bit 0) or a colptr segment (bit 1) was too small, or a sum
 *                     left the accumulators' range |sum| < 2^23 (bit 2; terms are assumed non-negative): outputs
 *                     invalid. */
/* Optional top-K cut of eps_expand_fill, a DEVICE-resident record: every candidate whose score exceeds `threshold`
 * is reported as (pos, val) -- pos = its index in the launch's candidate arrays -- in arrival order (sort by pos to
 * restore candidate order).  count (zeroed by the caller) may end above capacity: the list is then incomplete.
 * With a cut the score array itself is optional. */
typedef struct eps_score_cut {
    float threshold;
    uint32_t capacity;
    uint32_t count;
    uint32_t reserved;
    int64_t *pos;
    float *val;
} eps_score_cut;

int eps_expand_max_nodes(void);
int eps_expand_count(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t v_lo,
                     int64_t v_hi, const int32_t *col_order, int64_t *cand_count, void *stream);
int eps_expand_fill(const int64_t *rowptr, const int32_t *col, const float *val,
                    const float *node_w, int64_t n_nodes, int64_t v_lo, int64_t v_hi,
                    const int32_t *col_order, const int64_t *colptr, int64_t *cand_count,
                    int32_t *cand_u, int32_t *cand_v, int32_t *cn, float *score,
                    eps_score_cut *cut, void *workspace, int64_t workspace_bytes, void *stream);
/* eps_expand_fill with an explicit tile size (candidate ranks summed per LDS pass; 0 = the default 8192): results do not
 * depend on it -- small graphs are single-tile at the default, so the parity tests force several tiles per column. */
int eps_expand_fill_tiled(const int64_t *rowptr, const int32_t *col, const float *val,
                          const float *node_w, int64_t n_nodes, int64_t v_lo, int64_t v_hi,
                          const int32_t *col_order, const int64_t *colptr, int64_t *cand_count,
                          int32_t *cand_u, int32_t *cand_v, int32_t *cn, float *score,
                          eps_score_cut *cut, void *workspace, int64_t workspace_bytes,
                          int32_t tile_ranks, void *stream);
int64_t eps_expand_workspace_bytes(int64_t max_col_paths);
/* eps_expand_fill_tiled for SIGNED terms (cosine-weighted common neighbours: val = edge cosines in [-1, 1]): the same
 * exact 2^-40 fixed-point sums, without the in-kernel backstop that takes a negative sum for one that wrapped (status bit 2
 * is never set).  The caller guarantees the range: every |sum| < 2^22 (candidates.fused_score_bound, which sums |terms|,
 * is <= the largest degree for cosines).  A cut compares the raw sums with its threshold. */
int eps_expand_fill_signed(const int64_t *rowptr, const int32_t *col, const float *val,
                           const float *node_w, int64_t n_nodes, int64_t v_lo, int64_t v_hi,
                           const int32_t *col_order, const int64_t *colptr, int64_t *cand_count,
                           int32_t *cand_u, int32_t *cand_v, int32_t *cn, float *score,
                           eps_score_cut *cut, void *workspace, int64_t workspace_bytes,
                           int32_t tile_ranks, void *stream);

/* ---- K7+K1+K8: threshold scan of the whole candidate set (filter.py:96-142 + :160-161 under --keep_top) ------------
 * Computes the score of EVERY 2-hop non-edge of the given columns like eps_expand_fill does (same 2^-40 fixed-point
 * sums, bit-identical float32 scores) but writes neither the candidate list nor the score array: only the candidates
 * whose score exceeds out->threshold are reported.  Requires a SYMMETRIC adjacency with UNIT values (val == NULL;
 * filter.py's is: rank.py:33-35 for every dataset but collab) and exploits the symmetry: column v expands only the
 * endpoints u < v, so each unordered candidate pair {u, v} is scored once and reported once, as
 * key = (v << 32) | u with u < v; the caller mirrors it (the scores of (u,v) and (v,u) are equal term by term).
 *   eps_reverse_positions: revpos[e] for entry e of row v, w = col[e]: number of entries of row w below v (the position
 *                     of v in row w).  Per-graph table, int32[nnz].  The same pass can give half_paths[v] = sum of revpos
 *                     over row v (int64[N]: the two-hop half paths of column v = its work in the scan and the bound of
 *                     its survivors) and *asymmetric (device word, cleared by the call) = 1 if some entry (v, w) has no
 *                     mirror (w, v) -- the half scheme needs a symmetric pattern.
 *   eps_fixed_weights: fixw[i] = round(node_w[i] * 2^40): the per-node weights (eps_node_weights; all ones for the
 *                     common-neighbour count of models.py:536-542) in the accumulators' fixed point, int64[N].
 *   eps_filter_scan : columns = int32[n_columns] column ids in hand-out order (any subset, any order: a heaviest-first
 *                     order shortens the tail; a sample of columns estimates the bar; a rank's shard under
 *                     torch.distributed).  out is DEVICE-resident: threshold and capacity set by the caller, count
 *                     zeroed, key[] pre-filled with -1.  Slots are handed out in chunks, so after the launch the first
 *                     min(count, capacity) slots hold the survivors interleaved with untouched (-1) slots;
 *                     count > capacity means survivors were dropped.  max_degree: the longest row of the graph.
 *                     workspace: eps_filter_scan_workspace_bytes(max_degree) bytes of scratch (bucket records +
 *                     per-workgroup weight tables), 16-byte aligned. */
typedef struct eps_survivors {
    float threshold;
    uint32_t capacity;
    unsigned long long count;        /* slots handed out (64-bit: a list that overflows cannot wrap back under capacity) */
    int64_t *key;
    float *val;
    unsigned long long n_candidates; /* out (zeroed by the caller): unordered candidate pairs scored by the launch */
} eps_survivors;

int64_t eps_filter_scan_max_nodes(void);
int64_t eps_filter_scan_workspace_bytes(int64_t max_degree);
/* Id spaces wider than the LDS bitmap are scanned in id windows: eps_filter_scan_windows reports the window size / count
 * the launch will use for n_nodes ids, eps_row_window_splits fills the per-graph table it then needs:
 * splits[k * n_nodes + w] = number of entries of row w below id (k + 1) * win_ids, k = 0 .. n_win - 2 (int32). */
int eps_filter_scan_windows(int64_t n_nodes, int64_t *win_ids, int64_t *n_win);
int eps_row_window_splits(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t win_ids,
                          int64_t n_win, int32_t *splits, void *stream);
int eps_reverse_positions(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int32_t *revpos,
                          int64_t *half_paths_or_null, uint32_t *asymmetric_or_null, void *stream);
/* ---- per-graph tables built by the library (r04; csrc/graph_prep.hip): filter.py runs once per graph (submit_job.py:20-21), so
 * these are on the critical path of every run --------------------------------------------------------------------------------
 * eps_relabel_graph: the copy of a coalesced CSR graph under a node permutation -- row i of the copy = row perm[i] of the graph
 *   with every id x replaced by inv[x] (inv[perm[i]] = i, int32), rows sorted ascending again (a segmented radix sort over the
 *   id_bits bits of the ids; values travel with their entries).  new_rowptr = the caller's prefix sum of the degrees in perm
 *   order (int64[n_nodes + 1]).  workspace: eps_relabel_graph_workspace_bytes(n_nodes, nnz, with_values) bytes, 256-byte aligned.
 * eps_reverse_positions_symmetric: what eps_reverse_positions reports (revpos, half_paths = its row sums, *asymmetric) for a
 *   SYMMETRIC pattern with half the searches: entry (v, w), w > v, looks v up in row w and writes both its own position and --
 *   at the place it found v -- its mirror's.  On any other pattern *asymmetric comes back 1 and revpos is not usable.
 *   stats (optional, 3 DEVICE uint64): largest degree, largest half_paths[v], sum of half_paths -- the scalars the scan reads.
 * eps_score_bound: *bound (DEVICE double) = max over rows v of sum_w |A[v,w]| |node_w[w]| max_u |A[u,w]| in float64 (without
 *   stored values: sum of |node_w| over the row; node_w NULL: the degree) -- an upper bound of every fused score of the graph.
 *   workspace: n_cols uint32 with stored values, else may be NULL. */
int64_t eps_relabel_graph_workspace_bytes(int64_t n_nodes, int64_t nnz, int32_t with_values);
int eps_relabel_graph(const int64_t *rowptr, const int32_t *col, const float *val_or_null, const int64_t *perm, const int32_t *inv,
                      const int64_t *new_rowptr, int64_t n_nodes, int64_t nnz, int32_t id_bits, int32_t *out_col,
                      float *out_val_or_null, void *workspace, int64_t workspace_bytes, void *stream);
int eps_reverse_positions_symmetric(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t nnz, int32_t *revpos,
                                    int64_t *half_paths, uint32_t *asymmetric, unsigned long long *stats_or_null, void *stream);
/* eps_reverse_positions_sorted (r06): the same outputs without a search -- a stable radix sort of the entry indices by column id
 * puts the mirror of the CSR's j-th entry at place j (symmetric patterns), one pass scatters the positions and checks the
 * pattern on the way; id_bits = bits of the largest id; workspace: eps_reverse_positions_sorted_workspace_bytes() bytes,
 * 256-byte aligned.  (filter.py:96-109 leaves the adjacency as it loaded it; this table is the scan's: the position of v in
 * row w for every stored (v, w) -- what lets column v walk only the endpoints u < v of its rows.) */
int64_t eps_reverse_positions_sorted_workspace_bytes(int64_t n_nodes, int64_t nnz);
int eps_reverse_positions_sorted(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t nnz, int32_t id_bits,
                                 int32_t *revpos, int64_t *half_paths, uint32_t *asymmetric, unsigned long long *stats_or_null,
                                 void *workspace, int64_t workspace_bytes, void *stream);
/* eps_node_order: order[i] (int32) = the node with the i-th largest key, ties by ascending id (a stable descending radix sort)
 * -- keys = the degrees (rowptr given: the hubs-first labels) or keys[] (int64, non-negative: the scan's heaviest-first column
 * order from the half paths).  Optional by-products for eps_relabel_graph: perm64[i] = order[i], inv32[order[i]] = i,
 * new_rowptr[0 .. n] = exclusive prefix of the keys in that order.  workspace: eps_node_order_workspace_bytes(n) bytes, 256-byte
 * aligned. */
int64_t eps_node_order_workspace_bytes(int64_t n);
int eps_node_order(const int64_t *rowptr_or_null, const int64_t *keys_or_null, int64_t n, int32_t *order_or_null,
                   int64_t *perm64_or_null, int32_t *inv32_or_null, int64_t *new_rowptr_or_null, void *workspace,
                   int64_t workspace_bytes, void *stream);
int eps_score_bound(const int64_t *rowptr, const int32_t *col, const float *val_or_null, const float *node_w_or_null,
                    int64_t n_rows, int64_t n_cols, int64_t nnz, double *bound, void *workspace, void *stream);
int eps_fixed_weights(const float *node_w, int64_t n, int64_t *fixw, void *stream);
int eps_filter_scan(const int64_t *rowptr, const int32_t *col, const int32_t *revpos, const int64_t *fixw,
                    const int32_t *splits_or_null, int64_t n_nodes, int64_t nnz, int64_t max_degree,
                    const int32_t *columns, int64_t n_columns, eps_survivors *out, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* ---- the same threshold scan in ONE pass over the two-hop paths (r03) ------------------------------------------------------
 * csrc/scan_pieces.hip: the piece kernel -- its generic body and the lean body of the main launch's single-round columns (lean_from) --,
 * its planner and the launch (eps_scan_screen[_weighted], eps_scan_plan[_rewalk]);
 * csrc/scan_light.hip: the lean kernel of the main launch's light single-piece columns (launched by eps_scan_screen: light_from);
 * csrc/scan_tables.hip: the builders of the tables a launch reads (eps_scan_windows / _bounds / _cuts / _window_paths[_columns] /
 * _screen_weights / _row_sums / _row_records / _column_pack); csrc/rescore.hip: the exact re-scoring of the survivors
 * (eps_rescore_runs[_dev], eps_rescore_weighted).
 * Reports what eps_filter_scan reports -- key = (v << 32) | u, u < v, of every 2-hop non-edge of the given columns whose
 * score can exceed out->threshold (filter.py:96-142 + :160-161 under --keep_top) -- but a column is scored in PIECES (runs of
 * id windows of its endpoints) whose candidates each own a slot of an LDS table, so every path is read once and costs one
 * table update.  The table holds 32-bit SCREENING sums of weights rounded UP to 2^-shift fixed point: an upper bound of the
 * exact 2^-40 fixed-point score, so no candidate above the bar is lost and a few just below it pass as well; out->val holds
 * the screening score (sum * 2^-shift).  The caller re-scores the survivors exactly (eps_rescore_runs; for a graph with
 * stored values eps_rescore_weighted: int64 sums of the 2^-40 fixed-point terms, order-independent, bit-identical to
 * eps_filter_scan's sums) and drops those <= the bar.
 * Needs what eps_filter_scan needs (symmetric adjacency, revpos) plus max degree < 65536 and weights >= 0; unit-valued
 * adjacencies go through eps_scan_screen, adjacencies with stored values through eps_scan_screen_weighted.
 *   eps_scan_windows      : M, the number of id windows per graph (32).
 *   eps_scan_cuts         : cuts[w * M + k] = entries of row w with id < bounds[k + 1] (uint16; 16-byte aligned), for the
 *                           caller's window boundaries bounds[0 .. M] (bounds[0] = 0, bounds[M] = n_nodes, non-decreasing;
 *                           windows of equal stored-entry mass balance the pieces).  Per-graph table.
 *   eps_scan_window_paths : wpaths[v * M + k] = two-hop half paths of column v that end in id window k (uint32; exact, from
 *                           the cut table).  Per-graph table; mandatory since v6 (a launch used to sum them itself without).
 *   eps_scan_screen_weights: fx32[i] = max(1, ceil(fixw[i] / 2^(40 - shift))); *bad (device word, cleared by the call):
 *                           bit 1 a negative weight, bit 2 a weight that does not fit 32 bits.  shift must keep every
 *                           screening sum of the graph below 2^31 (bit 31 of a table word flags a known edge) (the caller's score bound: eps_amd.scan.screen_shift).
 *   eps_scan_screen       : out as for eps_filter_scan (slots are handed out in chunks: 8192 per request under a bar, 2 x table
 *                           slots -- 8192 / 16384 / 32768 for variant 2 / 0 / 1 -- without one, where a piece's whole yield
 *                           survives; a survivor beyond its workgroup's reservation takes a slot of its own);
 *                           ssum / smax (optional, both or neither; per graph and weight table): ssum[v] = sum of fx32 over
 *                           row v (any pair's screening sum is at most the smaller of its two endpoints' ssum), smax[k] =
 *                           the largest ssum among the ids >= bounds[k] (k = 0 .. M; smax[M] = 0).  With them, pieces whose
 *                           sums provably fit next to their key bits keep key and sum in ONE table word (twice the
 *                           candidates per piece); their weights drop up to shift - 8 low bits, rounded up (still an upper
 *                           bound; out->val stays in units of 2^-shift);
 *                           batch_from: columns[0 .. batch_from) are handed to the workgroups one at a time, the rest eight per
 *                           draw (the hand-out is an atomic on one word, ~11 ns each: light columns -- give the list
 *                           heaviest first -- would wait for it); n_columns or more, or negative: one at a time throughout;
 *                           variant (low byte) 0: 512 threads / 8192-slot table (2 workgroups per CU), 1: 1024 / 16384 (1), 2: 256 /
 *                           4096 (4); byte 1 of `variant` (eps_scan_plan and eps_scan_screen alike): 0, or dmax + 1 = a limit on
 *                           the low weight bits a packed / 16-bit direct piece may drop (default shift - 8).  Lower it when the
 *                           graph's smallest weight is small: the screening score exceeds the exact one by up to 2^d + 1 units
 *                           per path, and the pre-filter before the exact re-scoring is as sharp as that is small next to a weight;
 *                           bit 16 of `variant` (r06; eps_scan_screen, the 256-thread geometry, unit-valued graphs, a launch under a
 *                           bar): packed pieces of single-round columns run as SKETCH pieces -- no keys: every path adds its
 *                           weight to one slot of each of two half tables (two hashes, non-returning adds), a candidate's sum
 *                           is at most the smaller of its two slots (an UPPER bound: what a screen needs and no more, so the
 *                           reported sums are not exact even where hashed pieces' would be -- re-score), the ids that reach the
 *                           bar are reported once each from a second look at the piece's paths; the caller keeps 8192 x the heaviest
 *                           fx32 below 2^32 (a coarser `shift` if need be), so that no slot can wrap; bits 17..23: slots of the
 *                           per-workgroup set of reported ids (a power of two <= 64; 0 = 128); bit 24 (eps_scan_plan AND the
 *                           eps_scan_screen launch that uses the plan, together with bit 16): a packed piece of a column of
 *                           <= 256 rows holds up to 8192 paths -- without keys neither key bits, sum field nor table slots bound it;
 *                           *status (device word, cleared by the call): value 2 (bit 1) = a table filled up (results
 *                           invalid; cannot happen within the planner's piece limits: a backstop); value 8 (bit 3) = a sketch
 *                           piece had more ids to report than its set holds (results invalid: repeat the launch without
 *                           bit 16, on a plan without bit 24); value 16 (bit 4) = sketch pieces ran (informational). */
int32_t eps_scan_windows(void);
/* eps_rescore_runs (csrc/rescore.hip): exact scores of screened survivors.  keys = (u << 32) | v, sorted ascending (runs of equal u: the hubs
 * recur); fixw = eps_fixed_weights(node_w); out[i] = float32 of the exact int64 sum of the 2^-40 fixed-point weights over the
 * common neighbours of pair i -- bit-identical to eps_filter_scan's / eps_expand_fill's score.  Unit-valued adjacency.
 * eps_rescore_weighted: the same for an adjacency with stored values: term = (A[u,w] * A[v,w]) * node_w[w] in float32, each
 * converted to 2^-40 fixed point (eps_expand_fill's weighted score); keys in any order.
 * LIMIT of eps_rescore_runs and eps_rescore_runs_dev (not of eps_rescore_weighted, which indexes with 64 bits): col[] is addressed
 * with 32-bit byte offsets and 32-bit entry indices, like eps_scan_screen's -- the graph must hold FEWER THAN 2^30 stored
 * entries (rowptr[n_nodes] < 2^30).  The two calls take no nnz and cannot check it: the caller must (ops.rescore_runs[_dev]
 * refuse col.numel() >= 2^30; scan.scan_plausible keeps such graphs away from the scan altogether). */
int eps_rescore_runs(const int64_t *rowptr, const int32_t *col, const int64_t *fixw, int64_t n_nodes, const int64_t *keys,
                     int64_t n, float *out, void *stream);
int eps_rescore_weighted(const int64_t *rowptr, const int32_t *col, const float *val, const float *node_w, int64_t n_nodes,
                         const int64_t *keys, int64_t n, float *out, void *stream);
int eps_scan_cuts(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, const int32_t *bounds, uint16_t *cuts,
                  void *stream);
int eps_scan_screen_weights(const int64_t *fixw, int64_t n, int32_t shift, uint32_t *fx32, uint32_t *bad, void *stream);
int eps_scan_window_paths(const int64_t *rowptr, const int32_t *col, const int32_t *revpos, const uint16_t *cuts,
                          int64_t n_nodes, const uint32_t *heads_or_null, uint32_t *wpaths, void *stream);
/* eps_scan_window_paths_columns (r06): the rows of that table for the listed columns only (the other rows are left untouched; no
 * head table): what a launch without a plan table over a few columns -- the bar sample, filter.py:96-142 on every 512-th column --
 * needs, so that a one-shot run builds the whole-graph table and its plan only if a launch without skipped heads asks for them. */
int eps_scan_window_paths_columns(const int64_t *rowptr, const int32_t *col, const int32_t *revpos, const uint16_t *cuts, int64_t n_nodes,
                                  const int32_t *columns, int64_t n_columns, uint32_t *wpaths, void *stream);
int eps_scan_screen(const int64_t *rowptr, const int32_t *col, const int32_t *revpos, const uint32_t *fx32,
                    const uint16_t *cuts, const uint32_t *wpaths, const uint32_t *ssum_or_null,
                    const uint32_t *smax_or_null, const uint32_t *pptr_or_null, const uint32_t *plan_or_null,
                    const uint32_t *heads_or_null, const uint32_t *rowrec_or_null, const uint32_t *pack_or_null, const int32_t *bounds,
                    int64_t n_nodes, int64_t nnz,
                    const int32_t *columns, const uint32_t *colrec_or_null, int64_t n_columns, int64_t batch_from,
                    int64_t lean_from, int64_t lean_batch_from, int64_t light_from, int32_t shift,
                    int32_t variant, eps_survivors *out, uint32_t *status, void *stream);
/* lean_from (csrc/scan_pieces.hip, the LEAN body; light_from or more, or negative: no lean zone): columns[lean_from, light_from) are
 * SINGLE-ROUND columns -- at most 256 rows, every plan record direct (16- or 32-bit) or packed (it runs as a sketch piece), every
 * piece within one range of the unit bitmap (paths + 3 x rows <= 4 x 8192) -- and go through a body of the piece kernel compiled for
 * exactly that, in a launch of its own on the same stream between the piece kernel's over columns[0, lean_from) and the light
 * kernel's: the same pieces, list and status word, a ticket counter of its own; lean_batch_from counts within the zone as batch_from
 * does within columns[0, lean_from).  Under the same conditions as a light zone.  A column or piece outside the rule sets status
 * bit 1 and is left out (a backstop).
 * eps_scan_lean_blocks_per_cu: workgroups of that body a compute unit holds at its LDS size, as the runtime counts them (4 is what the
 * geometry is built for), or a negative error code. */
int eps_scan_lean_blocks_per_cu(void);
/* light_from (csrc/scan_light.hip; n_columns or more, or negative: no light zone): columns[light_from, n_columns) are LIGHT --
 * exactly one plan record, of the packed kind, at most 64 rows, paths + known edges <= 2048 -- and go one per WAVE through a lean kernel launched by the same call on the same stream, after the piece
 * kernel has run columns[0, light_from): the same sketch-piece semantics, the same list and status word, tickets of eight columns on
 * a counter of its own.  Only with the main launch's tables (plan, records, heads, pack) and bit 16 of `variant`; batch_from counts
 * within columns[0, light_from).  A column that does not meet the bounds sets status bit 1 and is left out (a backstop). */
/* pack (optional, r06; the main launch only: variant 2 with plan table, row / column records, heads and sum bounds; 16-byte
 * aligned): eps_scan_column_pack's table -- 32 bytes per stored entry (v, j) in CSR order: {col, rowptr[col] (low word), fx32[col],
 * revpos | cut of column v's FIRST piece in row col << 16} {the cuts of v's pieces 1..8 in that row, 16 bits each}.  A column of
 * at most 256 rows then sets up from ONE contiguous stream (a 16-byte load per row) instead of neighbour ids -> one 128-byte
 * row-record line per neighbour.  Built per (graph, weights, plan table): filter.py:96-142 reads no such table -- it is the scan's. */
int eps_scan_column_pack(const int64_t *rowptr, const int32_t *col, const int32_t *revpos, const uint32_t *rowrec, const uint32_t *pptr,
                         const uint32_t *plan, int64_t n_nodes, uint32_t *pack, void *stream);
/* colrec (optional; needs the plan table; 16-byte aligned): 8 words per entry of `columns`, in the same order -- {v, rowptr[v] (low
 * word), degree, heads[2 v], heads[2 v + 1], ssum[v], pptr[v], pptr[v + 1] - pptr[v]} (zeros where a table is absent) -- what a
 * column's set-up otherwise reads through a chain id -> five tables, as ONE 32-byte load at the hand-out index.  The caller builds
 * it with plain gathers (eps_amd.scan.column_records). */
/* eps_scan_row_records: rowrec[w * 32 + 0 .. 15] = the 32 cuts of row w, [16] = rowptr[w] (low word), [17] = fx32[w], rest 0 -- ONE
 * 128-byte line per node with everything eps_scan_screen gathers per walked row (r05: three gathers into three tables were 384
 * bytes of fabric traffic per row for 24 bytes wanted).  Per (graph, weight table); 128-byte aligned; optional for eps_scan_screen.
 * LIMIT: word 16 keeps the LOW 32 bits of rowptr[w], so the records are right only for a graph of fewer than 2^32 entries; the call
 * takes no nnz and cannot check it.  Their one reader, eps_scan_screen, refuses nnz >= 2^30; ops.scan_row_records refuses a stated
 * nnz >= 2^30 (eps_amd.scan passes col.numel()), and eps_amd.scan builds them only for a graph that passed scan_plausible. */
int eps_scan_row_records(const uint16_t *cuts, const int64_t *rowptr, const uint32_t *fx32, int64_t n_nodes, uint32_t *rowrec,
                         void *stream);
/* ---- skipped heads (r05; csrc/scan_heads.hip): half of all two-hop paths run through a few thousand hub rows whose weights are
 * the smallest there are, so under a bar a column need not walk them (still filter.py:96-142 + :160-161 under --keep_top) ------
 *   eps_scan_heads     : heads[2 v] = x_v, heads[2 v + 1] = T_v (uint32 pairs, 8-byte aligned): the longest prefix of row v with
 *                        ids < n_hub whose screening weights fx32 sum to T_v <= budget, at most max_rows (<= 65535) of them.  Built per
 *                        (graph, weight table, budget);
 *                        the budget is a fraction of the bar IN TABLE UNITS (bar x 2^shift).
 *   eps_scan_window_paths / eps_scan_plan / eps_scan_screen with heads: the column walks its rows from x_v on (window paths and
 *                        plan count those rows only; the three tables go together, and a head table needs the plan table built
 *                        for it), a table slot passes at bar - T_v, and out->val holds the WALKED sum as raw uint32 bits.
 *                        *status bit 2 (value 4): some T_v >= the bar in table units (the tables were built for a higher bar):
 *                        those columns were left out, the list is not valid.  A launch without a bar must not bring heads.
 *   eps_scan_hub_rows  : hubrows[w * words + (x >> 5)] bit (x & 31) = "x is a neighbour of w" for w < n_hub <= min(65536, n_nodes),
 *                        words = eps_scan_hub_row_words(n_nodes) (16-byte aligned rows): the adjacency rows of the first
 *                        n_hub ids as bitmaps over the id space.  Per-graph table (cleared and filled by the call).
 *   eps_scan_refine    : completes a walked list: every valid slot (key >= 0) of `walked` gets the exact head term -- the sum
 *                        of fx32[w] over the skipped rows w = col[rowptr[v] + j], j < x_v, that hold u (bit u of hub row w) -- added;
 *                        sums at or above out->threshold (in table units, as eps_scan_screen rounds it) are appended to `out`
 *                        (compact: out->count = their number; val = sum x 2^-shift) -- the list a launch without heads reports,
 *                        in another order.  out->count must be zeroed by the caller; out->n_candidates = walked->n_candidates
 *                        (the completed list stands for the launch that walked). */
int eps_scan_heads(const int64_t *rowptr, const int32_t *col, const uint32_t *fx32, int64_t n_nodes, int32_t n_hub,
                   uint32_t budget, int32_t max_rows, uint32_t *heads, void *stream);
int64_t eps_scan_hub_row_words(int64_t n_nodes);
int eps_scan_hub_rows(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int32_t n_hub, uint32_t *hubrows, void *stream);
int eps_scan_refine(const eps_survivors *walked, const uint32_t *heads, const uint32_t *hubrows, int32_t n_hub,
                    const uint32_t *fx32, const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int32_t shift,
                    eps_survivors *out, void *stream);
/* eps_scan_plan: the per-graph PLAN TABLE of eps_scan_screen -- every column's pieces, planned once by the scan kernel's own
 * planner (they depend on the graph, the window tables, the variant and, through ssum / smax, the weight table; not on the bar
 * or on the columns of a launch).  Two calls: with pptr / plan NULL it counts (pcount[v] = pieces of column v, uint32[n_nodes]);
 * the caller forms pptr = exclusive prefix sum (uint32[n_nodes + 1]) and calls again with plan = uint32[4 * pptr[n_nodes]]
 * (16-byte aligned; one 16-byte record per piece).  Pass the SAME wpaths / ssum / smax / shift / variant to eps_scan_screen
 * together with pptr / plan: a launch then reads a column's records instead of planning it (5 % of the launch).
 * d_used_or_null (fill call): the largest number of low weight bits any packed / 16-bit direct piece of the plan drops -- what
 * the caller's bound on (screening score - exact score) needs. */
/* eps_scan_bounds: the window boundaries eps_scan_cuts / eps_scan_screen expect -- bounds[0 .. M], M = eps_scan_windows(), windows
 * of equal stored-entry mass (bounds[k] = 1 + the first node whose row ends at or beyond k x nnz / M; non-decreasing).
 * eps_scan_row_sums: the per-node sum bounds of eps_scan_screen / eps_scan_plan: ssum[v] = min(2^31 - 1, sum of fx32 over row v),
 * smax[k] = the largest ssum among ids >= bounds[k] (k = 0 .. M; smax[M] = 0), *min_fx = the smallest fx32 of a node with at least
 * two neighbours (0xFFFFFFFF when there is none): (min_fx - 1) x 2^-shift is a floor under every path's exact term -- what bounds
 * the number of paths behind a screening sum.  workspace: M uint32. */
int eps_scan_bounds(const int64_t *rowptr, int64_t n_nodes, int32_t *bounds, void *stream);
int eps_scan_row_sums(const int64_t *rowptr, const int32_t *col, const uint32_t *fx32, const int32_t *bounds, int64_t n_nodes,
                      uint32_t *ssum, uint32_t *smax, uint32_t *min_fx, void *workspace, void *stream);
/* eps_scan_plan_rewalk: out2[0] = two-hop half paths that eps_scan_screen would walk AGAIN under this plan (hash-partitioned
 * passes of windows that are both wide and heavy), out2[1] = all half paths of the plan: what decides whether the one-pass
 * kernel suits a graph (eps_amd.scan.screen_variant). */
int eps_scan_plan_rewalk(const uint32_t *plan, int64_t n_rec, int32_t variant, unsigned long long *out2, void *stream);
int eps_scan_plan(const int64_t *rowptr, const uint16_t *cuts, const uint32_t *wpaths, const uint32_t *ssum_or_null,
                  const uint32_t *smax_or_null, const uint32_t *heads_or_null, const int32_t *bounds, int64_t n_nodes, int32_t shift,
                  int32_t variant, uint32_t *pcount, const uint32_t *pptr_or_null, uint32_t *plan_or_null, uint32_t *d_used_or_null,
                  void *stream);
/* eps_scan_screen_weighted: the scan on a SYMMETRIC adjacency WITH stored values (collab: rank.py:32-35 keeps the summed
 * multi-edge weights; val[e] must equal the value of e's mirror entry and be positive).  A path's term is
 * (A[u,w] * A[v,w]) * node_w[w] -- symmetric in (u, v), so the half scheme holds -- and its screening weight is formed per
 * path from the float values, rounded up.  node_w = the float32 node weights (no fx32 table); re-score with
 * eps_rescore_weighted.  The bar is taken rounded UP to a whole screening unit here (eps_scan_screen rounds it down, as
 * eps_scan_refine does): every reported out->val exceeds out->threshold, and no candidate above it is lost. */
int eps_scan_screen_weighted(const int64_t *rowptr, const int32_t *col, const float *val, const int32_t *revpos,
                             const float *node_w, const uint16_t *cuts, const uint32_t *wpaths, const int32_t *bounds,
                             int64_t n_nodes, int64_t nnz, const int32_t *columns, int64_t n_columns, int32_t shift,
                             int32_t variant, eps_survivors *out, uint32_t *status, void *stream);

/* ---- the candidate list of a block of columns of a graph WITHOUT stored values, on the scan kernel's structure ----------
 * Same results as eps_expand_count / eps_expand_fill above (filter.py:96-109: every 2-hop non-edge of columns
 * [v_lo, v_hi), column-major, u ascending; score = sum_w A[u,w] A[v,w] node_w[w] in 2^-40 fixed point, rounded once --
 * bit-identical), for unit-valued adjacencies: packed 64-entry units, 4-byte bucket records, one fixed-point weight per
 * (v, w) from a table (fixw = eps_fixed_weights(node_w); NULL with score == NULL: the list only).  col_order (optional)
 * = hand-out order, a permutation of range(v_hi - v_lo).  colptr[v_hi - v_lo + 1] = exclusive prefix of the counts
 * (or any upper-bound layout: the rest of a segment is padded with cand_u -1 / score -inf and cand_count, if given,
 * receives the real counts).  status: one device word, cleared by the call; after the stream has drained bit 1 = a
 * column outgrew its segment, bit 2 = a sum left the fixed-point range -- the outputs are then invalid.  splits /
 * max_degree / workspace as for eps_filter_scan (eps_filter_scan_workspace_bytes(max_degree) bytes).
 * revpos_or_null (eps_reverse_positions; symmetric pattern only): non-NULL selects the HALF list -- column v lists its
 * candidates u < v only, every unordered pair once -- for consumers that are symmetric in (u, v) themselves, like the
 * LinkPredictor decode of h_u * h_v (models.py:478-485): half the list, half the decode, the same scores. */
int eps_expand_unit_count(const int64_t *rowptr, const int32_t *col, const int32_t *revpos_or_null,
                          const int32_t *splits_or_null, int64_t n_nodes, int64_t nnz, int64_t max_degree, int64_t v_lo,
                          int64_t v_hi, const int32_t *col_order, int64_t *cand_count, void *workspace,
                          int64_t workspace_bytes, void *stream);
int eps_expand_unit_fill(const int64_t *rowptr, const int32_t *col, const int32_t *revpos_or_null, const int64_t *fixw,
                         const int32_t *splits_or_null,
                         int64_t n_nodes, int64_t nnz, int64_t max_degree, int64_t v_lo, int64_t v_hi,
                         const int32_t *col_order, const int64_t *colptr, int64_t *cand_count, int32_t *cand_u,
                         int32_t *cand_v, float *score, uint32_t *status, void *workspace, int64_t workspace_bytes,
                         void *stream);
/* eps_expand_unit_list (r06): the same list in ONE pass over the two-hop paths -- what filter.py:96-142 does once per candidate
 * -- without the counting launch and without a host read before the launch: colptr_ub[v_hi - v_lo + 1] is an exclusive
 * prefix of UPPER BOUNDS of the columns' candidate counts (min(two-hop paths of the column, n_nodes) always holds), column v
 * fills the front of [colptr_ub[v], colptr_ub[v + 1]) with its candidates (u ascending) and their scores -- the same values
 * as eps_expand_unit_fill, bit for bit --, cand_count[v] receives how many, and the rest of the segment is left unwritten
 * (no cand_v: the column of slot i is the segment that holds it).  status / workspace / splits / revpos_or_null as above. */
int eps_expand_unit_list(const int64_t *rowptr, const int32_t *col, const int32_t *revpos_or_null, const int64_t *fixw,
                         const int32_t *splits_or_null, int64_t n_nodes, int64_t nnz, int64_t max_degree, int64_t v_lo,
                         int64_t v_hi, const int32_t *col_order, const int64_t *colptr_ub, int64_t *cand_count,
                         int32_t *cand_u, float *score, uint32_t *status, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* ---- K4/K5: CSR x dense SpMM with fused epilogue -----------------------------------------
 * Replaces torch_sparse spmm_sum / spmm_mean inside GCNConv / SAGEConv (models.py:183-186,
 * :436-439) plus the bias add and the ReLU of the layer loop.
 *   mean == 0:  Y[i,:] = sum_k val[k] * X[col[k],:]
 *   mean != 0:  Y[i,:] = (sum_k X[col[k],:]) / max(rowlen(i), 1)      (values ignored)
 *   then  + bias[:] (if non-NULL), then ReLU (if relu != 0).
 * X is row-major [n_cols, ldx] (first f columns used), Y row-major [n_rows, ldy]. */
int eps_spmm_csr(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                 const float *x, int64_t ldx, int32_t f, const float *bias, int relu, int mean,
                 float *y, int64_t ldy, void *stream);

/* gcn_norm (torch_geometric 1.7.0 GCNConv, third-party): given A^ (diagonal already set to 1)
 * compute dis = rowsum^-1/2 (inf -> 0) and val_out[k] = (val[k]*dis[row])*dis[col[k]].
 * dis is an n_rows scratch/output buffer. */
int eps_gcn_norm(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                 float *dis, float *val_out, void *stream);

/* ---- dense f32 GEMM on the f32-input MFMA (exact f32) -------------------------------------
 * C[M,N] = act(A[M,K] * B[N,K]^T + bias[N] (+ C if accumulate)); B is row-major [N,K]
 * (torch.nn.Linear layout; GCNConv.weight [in,out] is passed transposed by the host).
 * Serves `x @ W` of GCNConv and lin_l / lin_r of SAGEConv (models.py:183, :436). */
int eps_gemm_f32(const float *a, int64_t lda, const float *b, int64_t ldb, const float *bias,
                 int relu, int accumulate, float *c, int64_t ldc, int64_t m, int32_t n, int32_t k,
                 void *stream);
/* `relu`: bit 0 = ReLU; bit 1 (value 2) = the product is symmetric and only the 128 x 128 tiles on and below the diagonal are
 * computed (the rest of C is left untouched).
 *
 * ---- common neighbours of a DENSE graph through the matrix cores (r05; csrc/dense_cn.hip) --------------------------------
 * filter.py:96-121 with CommonNeighborsPredictor('simple') (models.py:536-542) on a graph like ogbl-ddi (N = 4,267, 11.7 % of
 * all pairs are edges): CN = A A^T as one dense float32 product (exact below 2^24), the candidate list a masked read of it.
 *   eps_dense_adjacency : a[v * ld + w] = 1.0f for every stored entry, 0 elsewhere; the matrix has `rows` >= n_nodes rows of
 *                         ld >= n_nodes floats (padding rows / columns zero: the product's tiles want multiples of 128).
 *   eps_dense_candidates: the candidates of column v -- c[v * ld + u] > 0, a[v * ld + u] == 0, u < v (below_only: each unordered
 *                         pair once; c needs its lower tiles) or u != v (the reference's directed list; c needs all tiles) -- in
 *                         ascending u.  First call (colptr NULL): counts[v] = their number; the caller forms colptr = exclusive
 *                         prefix sum; second call: keys[colptr[v] + i] = (v << 32) | u, vals[..] = c[v * ld + u], and / or
 *                         rows[3 (colptr[v] + i) ..] = (float u, float v, count): the proposal file's row (filter.py:119).
 *   eps_dense_mirror_lower: c[u * ld + v] = c[v * ld + u] for u < v -- the upper triangle of a product computed with the triangle
 *                         flag, for readers that want whole rows. */
int eps_dense_adjacency(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t ld, int64_t rows, float *a,
                        void *stream);
int eps_dense_candidates(const float *a, const float *c, int64_t n_nodes, int64_t ld, int32_t below_only, int64_t *counts,
                         const int64_t *colptr_or_null, int64_t *keys_or_null, float *vals_or_null, float *rows_or_null,
                         void *stream);
int eps_dense_mirror_lower(float *c, int64_t n, int64_t ld, void *stream);

/* ---- K6: fused LinkPredictor decode ------------------------------------------------------
 * Replaces h[edges[0]], h[edges[1]] gathers (models.py:506) + LinkPredictor.forward
 * (models.py:478-485): out[p] = sigmoid(W_L ... relu(W_1 (h[u_p] (.) h[v_p]) + b_1) ... + b_L).
 * h: [n_nodes, hdim] row-major (ld = hdim).  w[l]: device pointers to row-major [out_l, in_l]
 * matrices (torch.nn.Linear layout), b[l]: [out_l]; hidden width == hdim for every hidden
 * layer, last layer out == 1.  w / b are HOST arrays of n_layers device pointers.
 * apply_sigmoid == 0 returns the pre-sigmoid logit.  Supported: hdim % 4 == 0, hdim <= 512,
 * 1 <= n_layers <= 8. */
int eps_mlp_decode(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                   const int32_t *v, int64_t n_pairs, const float *const *w,
                   const float *const *b, int32_t n_layers, int apply_sigmoid, float *out,
                   void *stream);

/* ---- K6b: the same decode on the bf16 matrix cores (screening precision) ---------------------
 * eps_mlp_decode_bf16 replaces the same call site as eps_mlp_decode -- LinkPredictor.forward (models.py:478-485) as the
 * filter stage calls it (filter.py:116-121) -- for callers that only have to FIND the best pairs: h is a bf16 table
 * [n_nodes, hdim] (uint16 bit patterns, row-major, 16-byte aligned), w[l] for l < n_layers - 1 are bf16 [hdim, hdim]
 * matrices, w[n_layers - 1] is the float32 [1, hdim] last layer, b[l] are float32 (hidden biases 16-byte aligned).
 * v_mfma_f32_32x32x16_bf16, fp32 accumulate.  Fixed rounding points (RNE): x0 = bf16(float(h_u) * float(h_v)); every hidden
 * layer adds its bias and applies ReLU in fp32, and all but the last are then rounded to bf16; the last hidden layer's
 * output, the final dot, the bias and the sigmoid are fp32.  out: float32 [n_pairs].
 * Supported: hdim % 16 == 0, hdim <= 256, 2 <= n_layers <= 8; anything else is EPS_EINVAL before any launch.
 * eps_f32_to_bf16 replaces nothing of the reference (which has no reduced precision): out[i] = the bf16 bits of x[i], RNE,
 * every NaN -> 0x7FC0 -- the bits of torch's float32 -> bfloat16; it prepares the table and the hidden weights of the call
 * above (models.py:478-485 through filter.py:116-121 again).
 * Both are additions, like eps_katz_* and eps_cos_* before them: no existing call changes, EPS_ABI_VERSION stays. */
int eps_mlp_decode_bf16(const uint16_t *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                        const int32_t *v, int64_t n_pairs, const void *const *w,
                        const float *const *b, int32_t n_layers, int apply_sigmoid, float *out,
                        void *stream);
int eps_f32_to_bf16(const float *x, int64_t n, uint16_t *out, void *stream);

/* ---- K6c: the same decode in TRAINING mode, forward and backward ---------------------------------
 * Replaces, in training mode, the h[edges[0]] / h[edges[1]] gathers (models.py:506), LinkPredictor.forward with dropout
 * (models.py:478-485: Hadamard -> (L-1) x [Linear, ReLU, dropout] -> Linear -> sigmoid) and what autograd records for them
 * (train_and_eval.py:31-96).  Domain of both calls: hdim % 4 == 0, 32 <= hdim <= 256, 2 <= n_layers <= 8; anything else is
 * EPS_EINVAL (the message names hdim= / n_layers=) before any launch; n_pairs == 0 succeeds without a launch.
 * Masks: uint32 [n_layers - 1][n_pairs][ceil(hdim / 32)], bit c & 31 of word c / 32 of row e belongs to unit c of edge e.
 *   keep  (in, or NULL = no dropout): a unit with its bit set is multiplied by keep_scale = 1 / (1 - p) AFTER the ReLU, any
 *         other unit becomes 0.
 *   taken (out, or NULL): set where the ReLU output is > 0, before dropout -- the branch the backward follows.
 * eps_mlp_decode_train: out float32 [n_pairs]; with keep == NULL the scores are eps_mlp_decode's, bit for bit.
 * eps_mlp_decode_backward: grad_out float32 [n_pairs] is dL/d(out); with apply_sigmoid the kernel multiplies by s (1 - s)
 * itself.  wt[l] (l < n_layers - 1): W_l transposed, row-major [in, out], 16-byte aligned.  Outputs, each nullable (grad_w /
 * grad_b are HOST arrays of n_layers device pointers, or NULL): grad_w[l] shaped like w[l], grad_b[l] like b[l], grad_h
 * float32 [n_nodes, hdim] (every row is written).  grad_h needs the incidence list of the batch: inc_order int32
 * [2 n_pairs] = the STABLE ascending argsort of the node ids cat(u, v), inc_ptr int64 [n_nodes + 1] = the first list
 * position of every node (inc_ptr[n_nodes] = 2 n_pairs); the incidences of a node are summed in list order (a self pair
 * u == v contributes twice: the derivative of h_u (.) h_u).  workspace: eps_mlp_decode_backward_workspace_bytes(...)
 * bytes, 16-byte aligned, contents arbitrary.  No atomics; every summation order is a function of the shapes (and of the
 * device's CU count) alone, so two calls on the same inputs return the same bits.
 * Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_mlp_decode_train(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                         const int32_t *v, int64_t n_pairs, const float *const *w,
                         const float *const *b, int32_t n_layers, const uint32_t *keep, float keep_scale,
                         int apply_sigmoid, float *out, uint32_t *taken, void *stream);
int64_t eps_mlp_decode_backward_workspace_bytes(int64_t n_pairs, int32_t hdim, int32_t n_layers);
int eps_mlp_decode_backward(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                            const int32_t *v, int64_t n_pairs, const float *const *w, const float *const *wt,
                            const float *const *b, int32_t n_layers, const uint32_t *keep, float keep_scale,
                            int apply_sigmoid, const float *grad_out, const int32_t *inc_order, const int64_t *inc_ptr,
                            float *const *grad_w, float *const *grad_b, float *grad_h, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ---- K6d: the training decode of DEA_GNN_JK: BatchNorm on batch statistics between Linear and ReLU -----
 * Replaces, in training mode, the decoder of the reference's DEA_GNN_JK.forward (models.py:118-128: Hadamard -> Linear(H, H)
 * -> BatchNorm1d on batch statistics -> ReLU -> dropout -> Linear(H, 1), a logit) and what autograd records for it
 * (train_and_eval.py:66-71).  Per channel c over the n_pairs edges: z = x0 W0^T + b0, mu = mean(z), var = the BIASED
 * variance, sigma = sqrt(var + eps), y = gamma (z - mu) / sigma + beta, a = relu(y) keep keep_scale, out = a . w1 + b1.
 * Domain of all three calls: hdim % 4 == 0, 32 <= hdim <= 256, n_layers == 2, 2 <= n_pairs < 2^30; anything else is
 * EPS_EINVAL (the message names hdim= / n_layers= / n_pairs=) before any launch (the workspace query returns 0).
 * w, b: HOST arrays of n_layers device pointers to the layers AS THEY ARE (w[0] = W0 [hdim, hdim], w[1] = w1 [1, hdim]).
 * eps_mlp_decode_bn_stats: mean, var float32 [hdim] of z over the batch (per-workgroup (count, mean, M2) triples in float64,
 *   merged in workgroup order).
 * The forward is eps_mlp_decode_train on the folded layer wf = diag(s) W0, bf = s b0 + beta - s mu, s = gamma / sigma,
 *   with apply_sigmoid = 0.
 * eps_mlp_decode_bn_backward: grad_out float32 [n_pairs] = dL/d(out).  wt[0]: W0 transposed; wf / bf: HOST arrays of
 *   n_layers - 1 pointers to the folded layer the forward ran on (the backward follows ITS ReLU branch); mean / var: what
 *   eps_mlp_decode_bn_stats returned.  Outputs, each nullable: grad_w[l] / grad_b[l] shaped like w[l] / b[l] (grad_b[0]
 *   is written as exact zeros: a bias in front of batch statistics has no gradient), grad_gamma, grad_beta float32 [hdim],
 *   grad_h float32 [n_nodes, hdim] with inc_order / inc_ptr and the incidence-order rule of eps_mlp_decode_backward.
 * workspace: eps_mlp_decode_bn_workspace_bytes(...) bytes (serves either call), 16-byte aligned, contents arbitrary.
 * No atomics; every summation order is a function of the shapes and the device's CU count: the same inputs give the same
 * bits.  Additions: no existing call changes, EPS_ABI_VERSION stays. */
int64_t eps_mlp_decode_bn_workspace_bytes(int64_t n_pairs, int32_t hdim, int32_t n_layers);
int eps_mlp_decode_bn_stats(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                            const int32_t *v, int64_t n_pairs, const float *const *w,
                            const float *const *b, int32_t n_layers, float *mean, float *var,
                            void *workspace, int64_t workspace_bytes, void *stream);
int eps_mlp_decode_bn_backward(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u,
                               const int32_t *v, int64_t n_pairs, const float *const *w, const float *const *wt,
                               const float *const *b, int32_t n_layers, const float *const *wf,
                               const float *const *bf, const float *gamma, const float *mean, const float *var,
                               float bn_eps, const uint32_t *keep, float keep_scale, const float *grad_out,
                               const int32_t *inc_order, const int64_t *inc_ptr, float *const *grad_w,
                               float *const *grad_b, float *grad_gamma, float *grad_beta, float *grad_h,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* ---- top-K selection with the declared tie rule ------------------------------------------
 * Replaces `all_scores[:,2].sort(descending=True)` (filter.py:160-161) for the K rows rank.py
 * ever reads (rank.py:294).  Declared order: score descending, then `id` ascending (== a stable
 * descending sort over the reference's candidate order; the reference's own torch.sort is
 * unstable on ties).  (score, id) is packed into an int64 whose SIGNED order realises the rule:
 *   key = (ordered_bits(score) ^ 0x80000000) << 32 | (0xFFFFFFFF - id),   id < 2^32,
 * so a plain descending sort / top-K / k-way merge of keys -- on one GPU or across shards --
 * gives the same result.  id = ids[i] if ids != NULL else id_base + i. */
/* k-th largest value of a float32 array (1 <= k <= n < 2^32) by radix select over the same order-preserving bit pattern:
 * the bar of the threshold scan and the cut of the final top-K need this one value, not a sorted array.  *kth (device)
 * receives it; torch.sort semantics for the order (-0 == +0; NaNs sort above +inf).  workspace:
 * eps_kth_largest_workspace_bytes() bytes, 8-byte aligned, contents arbitrary. */
int64_t eps_kth_largest_workspace_bytes(void);
int eps_kth_largest_f32(const float *x, int64_t n, int64_t k, float *kth, void *workspace, void *stream);
/* The same radix select in steps, for a vector that is spread over the ranks of a torch.distributed job (the bar of the
 * sharded scan, the final cut of filter.py:160-161 over all ranks' survivors).  state = eps_kth_largest_workspace_bytes()
 * bytes on the device, 8-byte aligned: { uint32 prefix, mask; uint64 k; uint32 hist[256] } (hist at byte 16).  Per round
 * (shift = 24, 16, 8, 0): eps_kth_hist_f32 adds the histogram of this rank's values (n may be 0), the caller sums hist over
 * the ranks (one all-reduce of 1 KiB), eps_kth_pick narrows the prefix and clears hist.  After the round with shift 0,
 * *out = the k-th largest of the union, -inf when the union holds fewer than k values. */
/* eps_select_compact: radix select + threshold + compaction of a short list in ONE launch (the selections of a filter step --
 * filter.py:160-161 keeps the K best rows -- were launch-latency bound: ten launches per select, one more per compaction).
 *   n = min(*n_dev_or_null, n_max): the slot counter of an eps_survivors list (eps_scan_screen marks the unused slots of its
 *   reservations "no survivor" itself, so a reader stops at the counter and the list needs no fill before the launch);
 *   entries with value -inf (and, when keys is given, key < 0) are no values;
 *   *kth = the k-th largest value, -inf when there are fewer than k (k == 0: -inf, nothing selected);
 *   *thr = mode 0: kth; mode 1: the largest float below kth (an inclusive bar for a scan that keeps scores above its
 *          threshold); mode 2: max(kth - pa, kth * pb) - |kth| * pc (a lower bound of the exact score behind a screening
 *          score: eps_amd.scan.Screen.lower_bound);
 *   out_keys / out_vals (out_cap entries each; both NULL: selection only) receive the entries with key >= 0 and value >= *thr in
 *   arbitrary order, *n_out (DEVICE int64) their number -- entries beyond out_cap are counted, not stored.  state: eps_select_compact_workspace_bytes() bytes, 8-byte aligned.
 * Single device; the sharded job-wide select stays eps_kth_begin / _hist_f32 / _pick with one all-reduce per round. */
int64_t eps_select_compact_workspace_bytes(void);
int eps_select_compact(const int64_t *keys_or_null, const float *vals, int64_t n_max, const unsigned long long *n_dev_or_null,
                       int64_t k, int32_t mode, float pa, float pb, float pc, float *kth_or_null, float *thr_or_null,
                       int64_t *out_keys_or_null, float *out_vals_or_null, int64_t out_cap, int64_t *n_out_or_null, void *state,
                       void *stream);
int eps_kth_begin(void *state, int64_t k, void *stream);
int eps_kth_hist_f32(const float *x, int64_t n, void *state, int32_t shift, void *stream);
int eps_kth_pick(void *state, int32_t shift, float *out_or_null, void *stream);
/* The k best DIRECTED proposals of a list of n unordered survivors of eps_filter_scan (keys v << 32 | u with u < v, one
 * entry per pair, no -1 slots; both orientations carry the pair's score), sorted by the declared rule -- score descending,
 * then key ascending (the reference's column-major candidate order): filter.py:160-161 for the rows rank.py:294 reads.
 *   eps_select_topk_cut : the pairs whose score reaches the ceil(k/2)-th best one, compacted into sel_keys / sel_vals
 *                         (n entries each, arbitrary order); *n_sel (DEVICE word) = their number m, which the caller reads.
 *   eps_select_topk_rows: those m pairs -> 2 m rows (v << 32 | u of proposal (u, v), score), sorted; the first
 *                         min(k, 2 m) go to out_keys / out_vals.  id_bits: every node id is below 2^id_bits.
 * workspaces: eps_select_topk_cut_workspace_bytes() / eps_select_topk_rows_workspace_bytes(m) bytes, 256-byte aligned. */
/* eps_compact_survivors: the survivors among the first n slots of an eps_survivors list (untouched slots keep key -1),
 * compacted in arbitrary order into out_keys / out_vals (n entries each); *n_out (DEVICE word) = how many.  workspace as for
 * eps_select_topk_cut. */
/* eps_select_topk_rows_relabelled: eps_select_topk_rows with the pairs' ids mapped through perm first (int64[n_nodes]: id i of a
 * relabelled, scanned graph is the caller's id perm[i]) -- rows and their order are in the caller's labels.
 * eps_sort_pairs_by_u: survivor keys v << 32 | u (u < v) -> u << 32 | v sorted by (u, v) (two stable radix sorts over the
 * id_bits bits of v, then of u): runs of equal u with ascending v, the input eps_rescore_runs wants.  v_block_shift > 0: by
 * (v >> v_block_shift, u, v) instead -- blocks of consecutive v first, so that concurrent workgroups of eps_rescore_runs stream
 * the same rows (0: off) -- WHEN the runs of equal (block, u) still average 64 pairs; otherwise the (u, v) order is returned
 * (eps_rescore_runs pays one bitmap of N(u) per run; counted and decided on the device).  workspace:
 * eps_sort_pairs_by_u_workspace_bytes(n) bytes, 256-byte aligned. */
/* eps_compact_between: the entries (key >= 0) whose score lies in [*lo, *hi) (DEVICE floats; either may be NULL: open end),
 * compacted in arbitrary order; *n_out (DEVICE int64) = how many.  A sharded filter step deals its final ordering over the
 * ranks by score range. */
int eps_compact_between(const int64_t *keys, const float *vals, int64_t n, const float *lo_or_null, const float *hi_or_null,
                        int64_t *out_keys, float *out_vals, int64_t *n_out, void *stream);
int eps_select_topk_rows_relabelled(const int64_t *sel_keys, const float *sel_vals, int64_t m, int64_t k, int32_t id_bits,
                                    const int64_t *perm, int64_t *out_keys, float *out_vals, void *workspace,
                                    int64_t workspace_bytes, void *stream);
/* eps_select_topk_rows_pairs (r06): the same rows written as the [2, k] proposal tensor rank.py:294 reads -- out_pairs[i] = u,
 * out_pairs[pairs_ld + i] = v (pairs_ld >= min(k, 2 m)) -- instead of packed keys; perm_or_null as in _relabelled. */
int eps_select_topk_rows_pairs(const int64_t *sel_keys, const float *sel_vals, int64_t m, int64_t k, int32_t id_bits,
                               const int64_t *perm_or_null, int64_t *out_pairs, int64_t pairs_ld, float *out_vals, void *workspace,
                               int64_t workspace_bytes, void *stream);
int64_t eps_sort_pairs_by_u_workspace_bytes(int64_t n);
int eps_sort_pairs_by_u(const int64_t *keys, int64_t n, int32_t id_bits, int32_t v_block_shift, int64_t *out_by_u, void *workspace,
                        int64_t workspace_bytes, void *stream);
int64_t eps_select_topk_cut_workspace_bytes(void);
int eps_compact_survivors(const int64_t *keys, const float *vals, int64_t n, int64_t *out_keys, float *out_vals,
                          int64_t *n_out, void *workspace, int64_t workspace_bytes, void *stream);
/* eps_compact_at_least: the survivors (key >= 0) among n slots whose score is at least *cut_or_null (a DEVICE float: the
 * job-wide cut from eps_kth_pick; NULL keeps every survivor), compacted in arbitrary order; *n_out (DEVICE int64, zeroed by
 * the call) = how many.  No workspace, no host round trip. */
int eps_compact_at_least(const int64_t *keys, const float *vals, int64_t n, const float *cut_or_null, int64_t *out_keys,
                         float *out_vals, int64_t *n_out, void *stream);
int eps_select_topk_cut(const int64_t *keys, const float *vals, int64_t n, int64_t k, int64_t *sel_keys, float *sel_vals,
                        int64_t *n_sel, void *workspace, int64_t workspace_bytes, void *stream);
int64_t eps_select_topk_rows_workspace_bytes(int64_t m);
int eps_select_topk_rows(const int64_t *sel_keys, const float *sel_vals, int64_t m, int64_t k, int32_t id_bits,
                         int64_t *out_keys, float *out_vals, void *workspace, int64_t workspace_bytes, void *stream);
/* ---- the tail of the filter step with DEVICE-side sizes (r06; csrc/tail_sort.hip) ------------------------------------------
 * What follows the scan under `--keep_top K` -- the pre-filter in front of the exact re-scoring, the cut, and the two orderings
 * of filter.py:160-161 for the K rows rank.py:294 reads -- without a host read in between: every count stays in device memory.
 *   state: eps_tail_state_bytes() bytes, 256-byte aligned, ZEROED once by the caller and owned by one stream; the kernels that
 *          consume it leave it zeroed (no memset launches per step).
 *   eps_score_hist: adds the histogram of a list's live scores (key >= 0 when keys are given, value > -inf and > *above_or_null)
 *          over order-preserving buckets of their distance to *base (DEVICE floats) to the state; n = min(*n_dev_or_null, n_max).
 *   eps_score_pick_compact: *kth = the lower edge of the highest bucket with at least k values at or above it (at most 2^-8 of the
 *          distance to *base below the exact k-th best value; -inf when fewer than k values or k == 0), *thr derived as
 *          eps_select_compact derives it (mode 0 / 1 / 2); the live entries with value >= *thr go to out_keys / out_vals
 *          (arbitrary order; swap_halves: key halves exchanged, v << 32 | u -> u << 32 | v and back), *n_out (DEVICE) = how many
 *          -- beyond out_cap counted, not stored.  Leaves the state's histogram zeroed.
 *   eps_radix_sort_by_u: the order eps_sort_pairs_by_u produces, in ONE cooperative launch, n read from the device.
 *   eps_radix_sort_rows: eps_select_topk_rows[_relabelled] in ONE cooperative launch, m read from the device; writes the
 *          proposal tensor itself: out_pairs[i] = u, out_pairs[out_ld + i] = v, out_scores[i] for the first min(k, 2 m) rows of
 *          the declared order; *n_rows_out_or_null (DEVICE) = that number.  workspace: eps_radix_sort_workspace_bytes(records)
 *          bytes (records = n_max resp. 2 m_max), 256-byte aligned.
 *   eps_rescore_runs_dev: eps_rescore_runs over min(*n_dev, n_max) pairs (the same limit: fewer than 2^30 stored entries). */
int64_t eps_tail_state_bytes(void);
/* eps_score_bins / eps_score_hist_into / eps_score_deal_plan: the same selection for a SHARDED step.  Every rank adds the histogram
 * of its re-scored scores to an array of its own (eps_score_bins() words, zeroed by the caller, the same *base on every rank) and
 * the arrays are all-gathered -- 25 KB per rank instead of its scores; eps_score_deal_plan then gives every rank, from the same
 * table hists[r * row_stride + bucket], the job-wide *cut (lower edge of the highest bucket with at least k values at or above it;
 * -inf when fewer), the world - 1 descending splitters[] of the final ordering (bucket edges: equal scores never straddle one;
 * range q = the selected scores in [splitters[q], splitters[q - 1]) holds about 1 / world of the selected pairs), counts[r * world
 * + q] = selected pairs of rank r in range q, and nsel[r] -- without another exchange.  filter.py:160-161 dealt over the ranks. */
int32_t eps_score_bins(void);
int eps_score_hist_into(const int64_t *keys_or_null, const float *vals, int64_t n_max, const unsigned long long *n_dev_or_null,
                        const float *base, const float *above_or_null, uint32_t *hist, void *stream);
int eps_score_deal_plan(const uint32_t *hists, int64_t row_stride, int32_t world, int64_t k, const float *base, float *cut,
                        float *splitters, int64_t *counts, int64_t *nsel, void *stream);
int eps_score_hist(const int64_t *keys_or_null, const float *vals, int64_t n_max, const unsigned long long *n_dev_or_null,
                   const float *base, const float *above_or_null, void *state, void *stream);
int eps_score_pick_compact(const int64_t *keys_or_null, const float *vals, int64_t n_max, const unsigned long long *n_dev_or_null,
                           const float *base, const float *above_or_null, int64_t k, int32_t mode, float pa, float pb, float pc,
                           int32_t swap_halves, float *kth_or_null, float *thr_or_null, int64_t *out_keys_or_null,
                           float *out_vals_or_null, int64_t out_cap, int64_t *n_out_or_null, void *state, void *stream);
int64_t eps_radix_sort_workspace_bytes(int64_t n_records);
int eps_radix_sort_by_u(const int64_t *keys, int64_t n_max, const int64_t *n_dev_or_null, int32_t id_bits, int32_t v_block_shift,
                        int64_t *out_by_u, void *workspace, int64_t workspace_bytes, void *state, void *stream);
int eps_radix_sort_rows(const int64_t *sel_keys, const float *sel_vals, int64_t m_max, const int64_t *m_dev_or_null, int64_t k,
                        int32_t id_bits, const int64_t *perm_or_null, int64_t *out_pairs, int64_t out_ld, float *out_scores,
                        int64_t *n_rows_out_or_null, void *workspace, int64_t workspace_bytes, void *state, void *stream);
int eps_rescore_runs_dev(const int64_t *rowptr, const int32_t *col, const int64_t *fixw, int64_t n_nodes, const int64_t *keys,
                         int64_t n_max, const int64_t *n_dev, float *out, void *stream);
/* ---- the K rows from one score sort of the re-scored pairs (csrc/rows_by_score.hip) ----------------------------------------------
 * The end of a one-rank step in one call, nothing read back: keys_by_u / vals are the n re-scored pairs as eps_rescore_runs leaves
 * them (u << 32 | v in the scanned graph's labels, any order).
 *   sorted_keys / sorted_vals (n entries): the list sorted by score, descending (order among equal scores unspecified), keys as
 *          v << 32 | u -- the first *n_sel of them are the selection eps_select_topk_rows[_pairs] takes;
 *   *cut, *n_sel (DEVICE): what eps_score_hist + eps_score_pick_compact give for this list with above = base = bar and k = k2 (live:
 *          score > *bar and > -inf; *cut = lower edge of the bucket of the k2-th best live score, -inf with fewer; *n_sel = live
 *          entries >= *cut) -- the same bits;
 *   out_pairs / out_vals: the first min(k, 2 *n_sel) rows of the declared order (score descending, then (v, u) ascending in the
 *          caller's labels: ids go through perm_or_null first) as out_pairs[i] = u, out_pairs[pairs_ld + i] = v, out_vals[i];
 *          pairs_ld >= min(k, 2 n).  Rows of equal score are ordered inside the kernel in runs of up to eps_rows_by_score_max_run()
 *          pairs; a longer run sets *flag (DEVICE int64: 0 / 1) and the rows of that call are void -- order sorted_keys[:*n_sel]
 *          with eps_select_topk_rows_pairs instead.  eps_rows_by_score_window(): sorted pairs per workgroup of that kernel.
 *          id_bits (1..32) is what the caller would hand eps_select_topk_rows_pairs: ids are compared as whole 32-bit words here.
 * workspace: eps_rows_by_score_workspace_bytes(n) bytes, 256-byte aligned. */
int32_t eps_rows_by_score_max_run(void);
int32_t eps_rows_by_score_window(void);
int64_t eps_rows_by_score_workspace_bytes(int64_t n);
int eps_rows_by_score(const int64_t *keys_by_u, const float *vals, int64_t n, const float *bar, int64_t k2, int64_t k, int32_t id_bits,
                      const int64_t *perm_or_null, int64_t *sorted_keys, float *sorted_vals, float *cut, int64_t *n_sel, int64_t *flag,
                      int64_t *out_pairs, int64_t pairs_ld, float *out_vals, void *workspace, int64_t workspace_bytes, void *stream);
int eps_pack_keys(const float *score, const int64_t *ids_or_null, int64_t id_base, int64_t n,
                  int64_t *keys, void *stream);
int eps_unpack_keys(const int64_t *keys, int64_t n, float *score_or_null, int64_t *id_or_null,
                    void *stream);

/* ---- Truncated Katz at pairs (csrc/katz_pairs.hip) --------------------------------------------
 * Replaces the collab branch of train_and_eval.py:272-343 (test_katz): `H = beta*A; H += beta*(A @ H)`
 * twice, read at the evaluation pairs -- without forming A^2 or A^3:
 *   out[p] = c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v]          (float64 accumulate, float32 result)
 * A is any square CSR [n_nodes x n_nodes] (values or NULL); rowptr_t / col_t / val_t is its transpose
 * (pass A's own pointers when A is symmetric).  paths_out = eps_two_path_counts(A), paths_in =
 * eps_two_path_counts(A^T) (the same array for a symmetric A): they decide, per pair, from which end the
 * three-hop walk starts.  u, v: int32[n_pairs] in [0, n_nodes).  workspace: device, 8-byte aligned,
 * contents arbitrary, eps_katz_workspace_bytes(n_pairs) bytes.  Bitwise deterministic. */
int eps_two_path_counts(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t *paths, void *stream);
int64_t eps_katz_workspace_bytes(int64_t n_pairs);
int eps_katz_pair_scores(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rowptr_t,
                         const int32_t *col_t, const float *val_t, const int64_t *paths_out, const int64_t *paths_in,
                         int64_t n_nodes, const int32_t *u, const int32_t *v, int64_t n_pairs, double c1, double c2,
                         double c3, void *workspace, float *out, void *stream);

/* ---- Truncated Katz over a block of columns (csrc/katz_columns.hip) -----------------------------
 * The filter's form of the score above: every candidate of column v shares y2 = (A^2)[:, v], so it is built once per
 * column (a keyed table, in LDS or in the workspace) and candidate u costs one pass over row u:
 *   out[p] = c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v]          (float64 accumulate, float32 result)
 * for candidate p = (cand_u[p], v), v the column of [v_lo, v_hi) whose range colptr[v - v_lo] .. colptr[v - v_lo + 1]
 * holds p (colptr: int64[v_hi - v_lo + 1], ascending from 0 to n_cand -- the column-major layout of the expansion).
 * Any u in [0, n_nodes) may be listed: stored edges, u == v and pairs without a walk of length <= 3 (exactly 0.0) too.
 * A, A^T as for eps_katz_pair_scores (val and val_t both NULL: unit-valued); paths_in = eps_two_path_counts(A^T).
 * max_support >= min(paths_in[v], n_nodes) for every column of the block: it sizes the workspace (device, 8-byte aligned,
 * contents arbitrary, eps_katz_columns_workspace_bytes(max_support) bytes -- 0 while every table fits LDS); a column
 * beyond it, or a cand_u outside the graph, scores NaN.  A score depends on the graph, the coefficients and the pair alone:
 * bitwise equal across launches, blocks and splits.  chunk: candidates per work unit, 0 for the default (a column with more
 * is scored by several units, each building its table again; any value in [1, 2^20] gives the same bits -- for measurements
 * and tests).  eps_katz_columns_limits (host only): the largest support bound whose table stays in LDS, and the smallest
 * default chunk; eps_katz_columns_chunk (host only): the default chunk of a list of n_cand candidates (longer lists take
 * larger units, which rebuild the tables of split columns less often). */
int eps_katz_columns_limits(int32_t *lds_capacity, int32_t *chunk);
int64_t eps_katz_columns_chunk(int64_t n_cand);
int64_t eps_katz_columns_workspace_bytes(int64_t max_support);
int eps_katz_column_scores(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rowptr_t,
                           const int32_t *col_t, const float *val_t, const int64_t *paths_in, int64_t n_nodes,
                           int64_t v_lo, int64_t v_hi, const int64_t *colptr, const int32_t *cand_u, int64_t n_cand,
                           double c1, double c2, double c3, int64_t max_support, int32_t chunk, void *workspace,
                           int64_t workspace_bytes, float *out, void *stream);

/* ---- Cosine-weighted common neighbours: the prologue (csrc/cosine_cn.hip) -------------------------------------------
 * Replaces the per-path cosines of models.py:556-575 ('simplecos' / 'mlpcos'): both factors of a path u - w - v depend
 * on one stored entry, so the score is the edge-valued common-neighbour sum over the graph whose values are
 *   eps_cos_node_features: xhat_i = x'_i / max(||x'_i||_2, 1e-8),  x' = x + (A @ x) / (rowsum(A) + 1e-6)
 *                          (A's values, or ones for val == NULL).  A square [n_rows x n_rows]; x float32 [n_rows x f]
 *                          with row stride ldx >= f (any f >= 1); xhat float32 [n_rows x ldh], ldh >= f -- a multiple of
 *                          32 floats (128-byte rows) is what the gathers want.  Columns [f, ldh) of xhat are written 0;
 *                          a row whose x' is zero gets a zero xhat row.
 *   eps_edge_cosines:      c[e] = xhat_row(e) . xhat_col(e) for every stored entry e (cosines ignore A's values).  xhat
 *                          as written above (ldh % 4 == 0, 16-byte aligned).  revpos (eps_reverse_positions of a
 *                          SYMMETRIC pattern) computes each undirected entry once and writes it to both positions; NULL
 *                          computes every entry (any pattern).
 * One wave per row, neighbour rows gathered whole; float32 throughout like the reference. */
int eps_cos_node_features(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                          const float *x, int64_t ldx, int32_t f, float *xhat, int64_t ldh, void *stream);
int eps_edge_cosines(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const float *xhat, int64_t ldh,
                     int32_t f, const int32_t *revpos, float *c, void *stream);

/* ---- ... and its backward, for training the embedding through the raw score (csrc/cosine_cn_bwd.hip) ---------------------
 * raw_p = sum_{w in N(u_p) & N(v_p)} c[(u_p, w)] * c[(v_p, w)]; with g_p = dL/draw_p the gradient reaches x in three steps:
 *   eps_cos_node_features_nrm:  eps_cos_node_features that also writes nrm[r] = max(||x'_r||_2, 1e-8) (float32 [n_rows]),
 *                               which the backward needs; xhat is the same, bit for bit.
 *   eps_pair_cn_backward:       gc[e] (float32 [nnz], aligned with col) = sum over the pairs p and their common neighbours w
 *                               of g_p * c[(v_p, w)] at e = (u_p, w) and g_p * c[(u_p, w)] at e = (v_p, w); a pair with
 *                               u == v adds both terms to the same entry, entries no pair reaches get 0.  c: the edge cosines
 *                               (|c| <= 2 is assumed).  The sums are 64-bit fixed-point integer atomics at a scale taken from
 *                               max |g_p| on the device (each term keeps >= 59 - ceil(log2(2 n_pairs)) bits below that
 *                               maximum), so gc is bit-identical from run to run and under any reordering of the pair
 *                               list.  Pairs with an id outside [0, n_rows) add nothing.  workspace: device memory, 8-byte
 *                               aligned, eps_pair_cn_backward_workspace_bytes(nnz) bytes; its contents need not survive.
 *   eps_cos_features_backward:  gxp[r] = (a_r - xhat_r (xhat_r . a_r)) / nrm[r], a_r = sum_{e = (r, w)} (gc[e] + gc[rev(e)])
 *                               xhat_w, rev(e) = rowptr[w] + revpos[e]; rows whose nrm is the clamp (<= 1e-8) get
 *                               a_r / 1e-8.  Always finite for finite inputs.  Needs a SYMMETRIC pattern and its revpos
 *                               (eps_reverse_positions).  gxs (or NULL) receives gxp[r] / (rowsum(A)_r + 1e-6) -- A's values, or
 *                               ones for val == NULL -- so that the smoothing's backward is gx = gxp + A @ gxs (eps_spmm_csr;
 *                               symmetric values).  xhat as eps_cos_node_features writes it; gxp / gxs float32 [n_rows x ldg],
 *                               ldg >= f, ldg % 4 == 0, 16-byte aligned; their columns [f, ldg) are written 0. */
int eps_cos_node_features_nrm(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                              const float *x, int64_t ldx, int32_t f, float *xhat, int64_t ldh, float *nrm, void *stream);
int64_t eps_pair_cn_backward_workspace_bytes(int64_t nnz);
int eps_pair_cn_backward(const int64_t *rowptr, const int32_t *col, const float *c, int64_t n_rows, int64_t nnz,
                         const int32_t *u, const int32_t *v, const float *g, int64_t n_pairs, float *gc, void *workspace,
                         int64_t workspace_bytes, void *stream);
int eps_cos_features_backward(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                              const float *xhat, int64_t ldh, int32_t f, const float *nrm, const int32_t *revpos,
                              const float *gc, float *gxp, float *gxs, int64_t ldg, void *stream);

/* ---- Adding a sorted batch of edges to a resident graph (csrc/csr_merge.hip) ---------------------------------------------
 * Replaces the adjacency rebuild of rank.py:28-36 (cat the training edges and the proposals, from_edge_index, to_symmetric)
 * for a graph that is resident already: the base (rowptr int64[n + 1], col int32 ascending per row, val float32 or NULL =
 * all ones; coalesced, square, n < 2^31) plus a batch xkeys int64[m], SORTED ascending, each row << 32 | col -- duplicates
 * allowed, both orientations of an undirected edge put in by the caller (a self pair twice, as to_symmetric makes it).  The
 * result is the coalesced sum: a stored pair keeps its place and gains the number of times the batch names it, a new pair
 * is inserted at its column's place with that number as its value.  Sorting the batch is the caller's job; nothing the size
 * of the graph is sorted.
 *   eps_csr_merge_count: new_deg[r] (int64[n]) = deg(r) + the distinct columns of row r's keys that the base row lacks (the
 *       row's keys are found by lower-bound searches on xkeys: no per-row pointer array).  xrank (int32[m + 1], out) is what
 *       eps_csr_merge_fill needs of the batch.  *status (DEVICE int32, cleared by the call): bit 1 = a key with row or col
 *       outside [0, n), bit 2 = xkeys not ascending; with a bit set the outputs mean nothing and the fill must not follow.
 *       workspace: eps_csr_merge_workspace_bytes(m) bytes, 256-byte aligned, contents arbitrary (m == 0: may be NULL).
 *   eps_csr_merge_fill:  new_rowptr (int64[n + 1]) = the exclusive prefix of new_deg (the caller's prefix sum), new_nnz its
 *       last entry; writes EVERY entry of new_col (int32[new_nnz]) and, when given, new_val (float32[new_nnz]): base value
 *       (1 for val == NULL) + multiplicity, resp. the multiplicity.  val and new_val both NULL: the pattern only.
 * EPS_EINVAL before any launch: n outside [0, 2^31) (the message names n=), m outside [0, 2^31 - 1) (m=), a null rowptr.
 * m == 0 launches nothing that reads xkeys and returns the base's degrees / arrays.  No atomics on the data: the same inputs
 * give the same bits.  Additions: no existing call changes, EPS_ABI_VERSION stays. */
int64_t eps_csr_merge_workspace_bytes(int64_t m);
int eps_csr_merge_count(const int64_t *rowptr, const int32_t *col, int64_t n, const int64_t *xkeys, int64_t m,
                        int64_t *new_deg, int32_t *xrank, int32_t *status, void *workspace, int64_t workspace_bytes,
                        void *stream);
int eps_csr_merge_fill(const int64_t *rowptr, const int32_t *col, const float *val_or_null, int64_t n, const int64_t *xkeys,
                       int64_t m, const int32_t *xrank, const int64_t *new_rowptr, int64_t new_nnz, int32_t *new_col,
                       float *new_val_or_null, void *stream);

/* ---- Segmented top-k: the k best entries of every segment of a score array (csrc/segment_topk.hip) ----------------------
 * filter.py --keep_per_node k: a block's candidates are column-major (column v, u ascending, one score each), so "node v's k
 * best proposals" is a top-k per segment.  Segment s is [colptr[s], colptr[s + 1]) of score (colptr int64[n_seg + 1], device),
 * or, with counts (int64[n_seg]) given, [colptr[s], colptr[s] + counts[s]): the padded upper-bound layout of a count-free
 * expansion -- nothing beyond the counted entries is read.  Order: ordered_bits(score) descending (the key of eps_pack_keys:
 * -0.0 ties +0.0), then position ascending.  outptr (int64[n_seg + 1], device) is the exclusive prefix of min(len_s, k): the
 * caller's, the kept count of a segment is known before any selection.  out_pos (int64[outptr[n_seg]]) receives POSITIONS
 * into the arrays, ascending within each segment; a segment of at most k entries keeps all of them.  order_or_null
 * (int32[n_seg]): the hand-out order of the segments, heaviest first (a permutation of 0 .. n_seg - 1); it decides the load
 * balance only, every segment is served whatever it holds; NULL = as numbered.
 * Selection by threshold (radix select of the k-th key on LDS histograms, then everything above it and the FIRST ties), in
 * ordered chunks: no resource depends on k, no atomics on global memory, the same inputs give the same bits.
 * eps_segment_topk_class_max(cls): the longest segment of work class cls -- 0: one wave, keys in registers; 1: one workgroup,
 * keys in LDS; longer segments are streamed once per radix round by one workgroup (-1 for any other cls).
 * EPS_EINVAL before any pointer is touched: k outside [1, 2^31) (the message names k=), n_seg outside [0, 2^31) (n_seg=), a
 * null colptr with n_seg > 0.  n_seg == 0 launches nothing.  Additions: no existing call changes, EPS_ABI_VERSION stays. */
int64_t eps_segment_topk_class_max(int32_t cls);
int eps_segment_topk(const int64_t *colptr, const int64_t *counts_or_null, const float *score, int64_t n_seg, int64_t k,
                     const int64_t *outptr, const int32_t *order_or_null, int64_t *out_pos, void *stream);

/* ---- Degree-normalised local indices (csrc/local_index.hip) -------------------------------------------------------------
 * The local indices of Zhou, Lu and Zhang ("Predicting missing links via local information") beside CN, AA and RA.  With
 * c = the number of common STORED neighbours of u and v (the pattern count: `count` of eps_pair_scores, `cn` of the
 * expansions; stored values are ignored) and a = rowptr[u + 1] - rowptr[u], b = rowptr[v + 1] - rowptr[v]:
 *   index 0 salton   c / sqrt(a b)      1 jaccard c / (a + b - c)     2 sorensen 2c / (a + b)     3 hpi c / min(a, b)
 *         4 hdi      c / max(a, b)      5 lhn     c / (a b)           6 pa       a b
 * A zero denominator scores 0.0.  float64 arithmetic on the integers, ONE rounding to float32: a score depends on
 * (c, a, b, index) alone, so score(u, v) == score(v, u) bit for bit and no block, slice or launch shape changes it.  An id
 * outside [0, n_nodes) scores NaN and touches nothing else.
 *   eps_local_index_pairs: score[p] of the pairs (u[p], v[p]) with their counts cn[p] (int32), p < n_pairs; any pair may be
 *       listed (stored edges, u == v, isolated nodes).
 *   eps_local_index_columns: a column-major block of the filter stage.  Slot p of the n_slots slots of cand_u belongs to
 *       column v = v_lo + s where segment s = [colptr[s], colptr[s + 1]) holds p (colptr int64[v_hi - v_lo + 1], ascending
 *       from 0 to n_slots) -- or, with counts (int64[v_hi - v_lo]), [colptr[s], colptr[s] + counts[s]): the padded layout of a
 *       count-free expansion, whose slots behind the counted entries are NEVER read and NEVER written.  The counts come as
 *       cn_i32 (int32) or cn_f32 (float32 holding the integer, n_nodes < 2^24): exactly one of the two.
 *       score_or_null (float32[n_slots]) receives every live slot's score.  bar_or_null (DEVICE float): the slots whose score
 *       EXCEEDS *bar are reported in ascending position -- surv_pos[i] (int64), surv_score[i], i < min(*n_surv, capacity);
 *       *n_surv (DEVICE int64) is the TRUE count, nothing is written past capacity (the caller then redoes the block with
 *       score_or_null).  NaN never exceeds a bar.  Three launches -- survivors per fixed slice of the slot array, one exclusive
 *       prefix, fill -- so the places do not depend on scheduling: no atomics, no workgroup waits on another.  workspace: with
 *       a bar, eps_local_index_columns_workspace_bytes(n_slots) bytes, 8-byte aligned, contents arbitrary; else unused.
 * EPS_EINVAL before any HIP call, the message naming the value: index outside [0, 7); both or neither count form; v_lo > v_hi
 * or columns outside [0, n_nodes]; a negative n_nodes / n_slots / capacity / workspace_bytes; n_nodes >= 2^24 with cn_f32; a
 * bar without n_surv (or without surv_pos / surv_score when capacity > 0); neither score nor bar; a workspace too small.
 * Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_local_index_pairs(const int64_t *rowptr, int64_t n_nodes, const int32_t *u, const int32_t *v, const int32_t *cn,
                          int64_t n_pairs, int32_t index, float *score, void *stream);
int64_t eps_local_index_columns_workspace_bytes(int64_t n_slots);
int eps_local_index_columns(const int64_t *rowptr, int64_t n_nodes, int64_t v_lo, int64_t v_hi, const int64_t *colptr,
                            const int64_t *counts_or_null, const int32_t *cand_u, int64_t n_slots,
                            const int32_t *cn_i32_or_null, const float *cn_f32_or_null, int32_t index, float *score_or_null,
                            const float *bar_or_null, int64_t capacity, int64_t *surv_pos, float *surv_score,
                            int64_t *n_surv, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Common-neighbour lists per pair, and their transpose (csrc/pair_cn_list.hip) --------------------------------------------
 * What Neural Common Neighbor (Wang, Yang, Zhang) adds to a GNN link decoder: z_b = sum of h_w over w in N(u_b) & N(v_b).  The
 * intersection kernels above only reduce over it; these hand it back as the CSR incidence C [n_pairs x n_rows] ("w is a common
 * STORED neighbour of pair b": the pattern only, stored values are ignored), so that Z = C H and dH = C^T dZ are eps_spmm_csr
 * with val == NULL -- sequential adds in entry order.  The graph: rowptr int64[n_rows + 1], col int32 strictly ascending per row.
 *   eps_pair_cn_list_count: count[b] (int32) = |N(u_b) & N(v_b)|.  A pair with an id outside [0, n_rows) counts 0 and reads
 *       nothing; u == v counts the whole row.
 *   eps_pair_cn_list_fill:  ptr (int64[n_pairs + 1]) = the exclusive prefix of count (the caller's); the common neighbours of
 *       pair b go to out_w[ptr[b] .. ptr[b + 1]), ASCENDING in w whichever row is the shorter one: the lists of (u, v) and (v, u)
 *       are the same array.  Count and fill are one kernel template in two modes, so they agree on what a match is; and whatever
 *       ptr holds, nothing is stored at or past ptr[b + 1], nor at or past ptr[n_pairs].  *status (DEVICE int32, cleared by the
 *       call) becomes 1 when a segment's length is not its pair's count (it would overflow, or stays short): the list then means
 *       nothing.  Plain stores only; the one atomic is the ticket that hands 64-pair chunks to the waves.
 *   eps_pair_cn_list_limits (host only): the long-row entries staged in LDS per pass, and the ratio long / short from which a
 *       long row beyond that capacity is searched in place -- the sizes at which the kernel changes its path.
 *   eps_cn_list_transpose:  the same incidence by node.  m = ptr[n_pairs] (the caller knows it: it sized out_w); every out_w in
 *       [0, n_rows).  tptr (int64[n_rows + 1]), tb (int32[m]): the pairs that list w are tb[tptr[w] .. tptr[w + 1]), ASCENDING in
 *       b (a stable radix sort of (w, b) by w; tptr by search).  A function of the input alone: no atomics.  Whatever out_w
 *       holds, every tb lies in [0, n_pairs) and every tptr in [0, m].  m == 0 clears tptr and reads nothing.  workspace:
 *       eps_cn_list_transpose_workspace_bytes(m, n_rows) bytes, 256-byte aligned, contents arbitrary (m == 0: may be NULL).
 * EPS_EINVAL before any launch: a negative size, n_rows / n_pairs / m >= 2^31, a null pointer that would be read or written.
 * n_pairs == 0 launches nothing.  Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_pair_cn_list_limits(int32_t *cap, int32_t *inplace_ratio);
int eps_pair_cn_list_count(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *u, const int32_t *v,
                           int64_t n_pairs, int32_t *count, void *stream);
int eps_pair_cn_list_fill(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *u, const int32_t *v,
                          int64_t n_pairs, const int64_t *ptr, int32_t *out_w, int32_t *status, void *stream);
int64_t eps_cn_list_transpose_workspace_bytes(int64_t m, int64_t n_rows);
int eps_cn_list_transpose(const int64_t *ptr, const int32_t *out_w, int64_t m, int64_t n_pairs, int64_t n_rows, int64_t *tptr,
                          int32_t *tb, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Local-community indices (csrc/local_community.hip) ------------------------------------------------------------------------
 * The local-community paradigm of Cannistraci, Alanis-Lobato and Ravasi (Sci. Rep. 3:1613, 2013): a pair is scored by the links
 * AMONG its common neighbours.  For a pair (u, v): L = the ascending list of the common STORED neighbours of rows u and v (the
 * lists above; stored values are ignored), c = |L|, a and b the stored entries of rows u and v, d_w those of row w,
 *   gamma(w) = |{z in L : z != w, z stored in row w}| for w in L  (the local-community degree; a self loop never counts)
 *   G = the sum of gamma over L, an integer (twice the links among the common neighbours on a symmetric pattern; symmetry is
 *       not required), LCL = G / 2, exact in float64.
 *   index 0 car  c LCL                                       1 cpa  ((a - c) + CAR) ((b - c) + CAR)
 *         2 caa  sum over L of gamma(w) / log2(d_w)          3 cra  sum over L of gamma(w) / d_w
 *         4 cjc  CAR / (a + b - c), 0.0 over a zero denominator
 * A term with gamma(w) == 0 is skipped (d_w = 1 never divides by log2 1).  float64 arithmetic on the integers, ONE rounding to
 * float32.  The two sums run over the list positions in a fixed association that depends on the list's length alone: blocks of
 * 64 consecutive entries, inside a block the balanced pairwise tree x[i] + x[i ^ 1], then ^ 2, ^ 4 ... (places past the end
 * hold 0.0), the blocks added first to last.  A score is therefore a function of (list, gamma, degrees, index): score(u, v) ==
 * score(v, u) bit for bit, whatever launch, batch position or route formed it.  c < 2 gives G = 0: car, caa, cra, cjc are 0
 * and cpa is (a - c)(b - c).
 *   eps_local_community_degrees: ptr (int64[n_pairs + 1]) and w (int32[ptr[n_pairs]]) are ANY strictly ascending segments of
 *       node ids (common-neighbour lists are the use; the kernel does not require it).  gamma[i] (int32) = the number of stored
 *       entries of row w[i] that occur in the segment holding i, other than w[i] itself.  A segment that does not ascend
 *       strictly, holds an id outside [0, n_rows), or whose bounds do not ascend inside [0, ptr[n_pairs]] sets *status (DEVICE
 *       int32, cleared by the call) to 1; its entries get gamma 0 and no row is read for them; other segments are unaffected.
 *       Nothing is read or stored at or past ptr[n_pairs].  Plain stores only; the one global atomic is the ticket that hands
 *       chunks of up to 64 segments to the waves; the counts are integers, so no result depends on an order or a launch shape.
 *   eps_local_community_limits (host only): the list length up to which the ordered pairs of a list are dealt over the lanes,
 *       the list entries staged in LDS per pass, and the ratio row / staged entries from which a row is searched in place --
 *       the sizes at which the kernel changes its path.
 *   eps_local_community_scores: score[p] (float32) of the pairs (u[p], v[p]): c from ptr, a and b from rowptr, G and the sums
 *       from (w, gamma, rowptr).  w == NULL and gamma == NULL together: nothing is listed, ptr carries the counts alone and
 *       every pair gets its closed form with G = 0 (the pairs with c < 2 of a batch).  An id of u, v outside [0, n_rows) scores
 *       NaN; an id of w outside it contributes no term and reads nothing.
 * EPS_EINVAL before any launch: a negative size, n_rows >= 2^31, index outside [0, 5), a null pointer that would be read or
 * written, w and gamma not both given or both NULL.  n_pairs == 0 launches nothing.  Additions: no existing call changes,
 * EPS_ABI_VERSION stays. */
int eps_local_community_limits(int32_t *short_max, int32_t *cap, int32_t *inplace_ratio);
int eps_local_community_degrees(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *ptr, const int32_t *w,
                                int64_t n_pairs, int32_t *gamma, int32_t *status, void *stream);
int eps_local_community_scores(const int64_t *rowptr, int64_t n_rows, const int32_t *u, const int32_t *v, const int64_t *ptr,
                               const int32_t *w, const int32_t *gamma, int64_t n_pairs, int32_t index, float *score, void *stream);

/* ---- Subgraph sketches (csrc/sketch.hip) ----------------------------------------------------------------------------------------
 * ELPH / BUDDY (Chamberlain et al., "Graph Neural Networks for Link Prediction with Subgraph Sketching", ICLR 2023): every node
 * carries a HyperLogLog sketch (256 one-byte registers) and a MinHash sketch (128 uint32 words) of its k-hop neighbourhoods, and a
 * pair's structural counts are estimated from those rows at a cost that depends on no degree.  All arithmetic here is integer.
 *   mix64(x) = the splitmix64 finaliser: z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *              z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (mod 2^64)
 *   own sketch of id x: h = mix64(x), register h >> 56 holds rank = clz32((h >> 24) & 0xFFFFFFFF) + 1 (33 for a zero word), the
 *              other 255 hold 0; word j = the low 32 bits of mix64(x ^ (j + 1) << 32).
 *   the empty set: registers 0, words 0xFFFFFFFF.  Union: byte-wise max of the registers, word-wise min of the words.
 * Tables: hll uint8 [., n, 256], mh uint32 [., n, 128], 16-byte aligned.
 *   eps_sketch_limits (host only): the row length above which eps_sketch_propagate reduces a row piecewise on several waves, and
 *       the pairs one wave of eps_sketch_pair_stats handles.
 *   eps_sketch_own: rows 0 .. n - 1 of hll / mh = the own sketches of the ids first_id .. first_id + n - 1 (ids below 2^31).
 *   eps_sketch_propagate: out[v] = the union of in[w] over the stored entries w of row v (rowptr int64[n_rows + 1], col int32[nnz],
 *       a square graph: the pattern only), and with keep_own != 0 also of in[v].  A row without entries gives the empty sketch
 *       (in[v] under keep_own).  An entry outside [0, n_rows) is skipped and reads nothing; row bounds are clamped to [0, nnz].
 *       No atomics: a function of the sets alone.  workspace: eps_sketch_propagate_workspace_bytes(nnz) bytes, 256-byte aligned,
 *       contents arbitrary (the partial unions of the rows longer than the limit; nnz == 0: may be NULL).
 *   eps_sketch_pair_stats: hll [K, n_rows, 256], mh [K, n_rows, 128], hop k at index k - 1.  stat int64 [n_pairs, K, K]: for
 *       (i, j) and M = the byte-wise max of hll[i][u] and hll[j][v],
 *         bits 0..41  S = sum over the registers of 2^(33 - M_r)   (a register above 33 adds nothing)
 *         bits 42..50 Z = #{r : M_r == 0}        bits 51..58 = #{t : mh[i][u][t] == mh[j][v][t]}
 *       A pair with an id outside [0, n_rows) gets -1 in all its slots and reads nothing.  Every slot of stat is written.
 * EPS_EINVAL before any HIP call: a null pointer, K outside {1, 2}, a negative size, first_id + n > 2^31, n_rows > 2^31, a
 * misaligned table, hll_out / mh_out overlapping their inputs.  Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_sketch_limits(int32_t *row_chunk, int32_t *pairs_per_wave);
int eps_sketch_own(int64_t first_id, int64_t n, uint8_t *hll, uint32_t *mh, void *stream);
int64_t eps_sketch_propagate_workspace_bytes(int64_t nnz);
int eps_sketch_propagate(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t nnz, const uint8_t *hll_in,
                         const uint32_t *mh_in, uint8_t *hll_out, uint32_t *mh_out, int keep_own, void *workspace,
                         int64_t workspace_bytes, void *stream);
int eps_sketch_pair_stats(const uint8_t *hll, const uint32_t *mh, int K, int64_t n_rows, const int32_t *u, const int32_t *v,
                          int64_t n_pairs, int64_t *stat, void *stream);

/* ---- The sizes at which the pair-score and re-scoring kernels change their path (host only) --------------------------------------
 * Each call returns the `#define`s of its unit, so that tests place rows, lists and id spaces ON the switch points and follow
 * a retuned constant; a NULL pointer skips that value.  Nothing is launched.
 *   eps_pair_scores_limits (csrc/pair_intersect.hip): small_max = the longer row of a pair up to which the pair is scored by
 *       sixteen lanes, four pairs a wave (unit values, float32 weights); cap = long-row entries staged in LDS per pass; queue =
 *       the slots of a wave's queue of deferred weight gathers (flushed before a 64-entry slice when more than queue - 64 are
 *       taken); inplace_ratio = long / short from which a row beyond cap is searched in place; ticket = consecutive 64-pair
 *       chunks per ticket of the launch that scores the longer pairs; cls_stride = every cls_stride-th 64-pair chunk is sampled
 *       by the classifier that picks the launch shape on the device (split when at least 60 % of the sampled pairs are small).
 *   eps_pair_scores_grouped_limits (csrc/pair_grouped.hip): chunk = pairs per workgroup chunk; queue = the slots of a wave's hit
 *       queue (flushed before a 256-entry unit when more than queue - 256 are taken); bitmap_bits = the bits of the LDS bitmap: an id
 *       space beyond it is hashed into it and every positive verified (so is one whose exact bitmap would leave no room for the
 *       queues beside it: the last sweep of ids below bitmap_bits); ring = rows a wave keeps in flight.
 *   eps_rescore_limits (csrc/rescore.hip): window_bits = ids per bitmap window of eps_rescore_runs; short_max = the row length of
 *       u up to which a pair goes to the short-row launch; chunk = pairs per workgroup chunk.
 * Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_pair_scores_limits(int32_t *small_max, int32_t *cap, int32_t *queue, int32_t *inplace_ratio, int32_t *ticket,
                           int32_t *cls_stride);
int eps_pair_scores_grouped_limits(int32_t *chunk, int32_t *queue, int32_t *bitmap_bits, int32_t *ring);
int eps_rescore_limits(int32_t *window_bits, int32_t *short_max, int32_t *chunk);

/* ---- Personalized PageRank by a fixed-point push (csrc/ppr_push.hip) ---------------------------------------------------------------
 * The forward push of Andersen, Chung and Lang in integers and synchronous rounds, so that the result is a function of (graph,
 * source, a16, thr, max_rounds) alone -- bitwise equal across launches, splits and table paths, and to a numpy truth.
 *   Graph: square CSR, the pattern only (stored values are not read).  Row u = the nodes u pushes to, d(u) its length.
 *   Mass is in units of 2^-48 (ONE = 2^48).  alpha = a16 / 65536, 1 <= a16 <= 32768.  thr = T = ceil(eps * 2^48), 1 <= T <= 2^48.
 *   Per source s: r[s] = ONE, everything else 0.  d(s) == 0: p[s] = ONE, no rounds.  While fewer than max_rounds rounds have run:
 *     F = { u : d(u) > 0 and r[u] >= T d(u) } on the state at the start of the round (T d(u) in exact integers: a product beyond
 *     ONE admits nothing; a node without entries has nowhere to push and keeps its residual); stop when F is empty; for u in F,
 *     R = r[u]: keep = (R * a16) >> 16, spread = R - keep, share = spread / d(u) (floor), p[u] += keep, r[u] = spread - share d(u),
 *     every entry w of row u receives share; the shares are added to r after every node of F has been reset.
 *   sources int32[n_sources] (duplicates allowed); qptr int64[n_sources + 1] ascending from 0; qnode int32[qptr[n_sources]]: the
 *   query nodes of every source.  Out, per query: mass = p[x] of its source (0 for a node never touched, or outside the graph);
 *   per source: rounds, pushes = sum |F|, steps = sum over the pushes of d(u), capped = 1 when the loop ended at max_rounds with
 *   a non-empty F; table_used (may be NULL) = 0 when the source's table stayed in LDS, 1 when it was redone in the workspace.
 *   sum p + sum r == ONE exactly.  thr * (65536 - a16) >= 65536 is required (a share could be 0 otherwise).
 *   Tables: a source that touches more than lds_nodes nodes is redone from the start in its workgroup's region of `workspace`
 *   (device, 8-byte aligned, contents arbitrary), a table of table_nodes keys: min(n_nodes, a bound on the touched nodes) never
 *   fills.  force_global != 0 skips the LDS attempt (same bits).  The launch takes min(2 per CU, n_sources, workspace_bytes /
 *   bytes per group) workgroups.  A graph of at most lds_nodes nodes without force_global needs no workspace.
 *   status int32[1], zeroed by the caller: bit 0 = a global table filled up (that source has rounds = -1 and mass 0: never a
 *   silent loss), bit 1 = a source left LDS without a workspace, bit 2 = a source outside the graph (rounds = -1), bit 3 = an
 *   entry of col outside the graph was skipped.
 * eps_ppr_push_limits (host only): lds_nodes = the keys the LDS table takes, big_row = the row length above which a row is walked
 * by the whole workgroup, groups_per_cu, and the workspace bytes per workgroup of a table of table_nodes keys (0 for 0).
 * EPS_EINVAL before any HIP call: a null pointer, a16 or thr out of range, thr too small for a16, max_rounds < 1, a negative or
 * oversized size, a workspace that is null, misaligned or smaller than one workgroup's region where one is needed.
 * Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_ppr_push_limits(int64_t table_nodes, int32_t *lds_nodes, int32_t *big_row, int32_t *groups_per_cu,
                        int64_t *workspace_bytes_per_group);
int eps_ppr_push(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, const int32_t *sources, int64_t n_sources,
                 const int64_t *qptr, const int32_t *qnode, int32_t a16, int64_t thr, int32_t max_rounds, int32_t force_global,
                 int64_t table_nodes, void *workspace, int64_t workspace_bytes, int64_t *mass, int32_t *rounds, int64_t *pushes,
                 int64_t *steps, int32_t *capped, int32_t *table_used, int32_t *status, void *stream);

/* ---- graph attention aggregate (GATConv; csrc/gat_attend.hip) ---------------------------------------------------------------
 * eps_gat_aggregate: rows [row0, row0 + n_rows) of
 *     out[i,h,:] = sum_{j in N(i) + {i}} alpha_ijh z[j,h,:]  (+ bias, then ReLU),
 *     alpha_i.h = softmax_j e_ijh,   e_ijh = LeakyReLU_slope(s_src[j,h] + s_dst[i,h]),
 *   N(i) = the stored entries of row i with col != i, plus i itself exactly once (stored values are not read; an empty row gives
 *   z[i] + bias exactly).  rowptr int64[n_rows + 1]: the row block's ABSOLUTE offsets into col (the slice rowptr[row0 .. row0 +
 *   n_rows] of the graph's); col int32, every id < n_nodes; z float32 [n_nodes, ldz], its first f columns read as [heads, C],
 *   C = f / heads; s_src / s_dst float32 [n_nodes, lds], their first `heads` columns read (two column blocks of one table are
 *   fine); bias float32[f] or NULL; out float32 [n_rows, ldo]; lse float32 [n_rows, heads] or NULL: m + log(sum_j exp(e - m)), the
 *   row's log-sum-exp per head, what the backward needs.  The maximum is subtracted before exp: scores of any magnitude give
 *   finite output.  Summation order: the self loop first, then the stored entries in stored order, sequentially -- the same bits
 *   on every call and from every row block.
 * eps_gat_aggregate_backward: the whole (square, SYMMETRIC-pattern) graph.  With alpha_ij = exp(e_ij - lse_i), D_ih =
 *   <gout[i,h,:], out_nobias[i,h,:]> and ds_ij = alpha_ij (<gout[i,h,:], z[j,h,:]> - D_ih) (raw_ij > 0 ? 1 : slope):
 *     gz[j] = sum_i alpha_ij gout[i],   g_s_src[j,h] = sum_i ds_ij,   g_s_dst[i,h] = sum_j ds_ij
 *   (g_s_src / g_s_dst float32 [n_nodes, heads] contiguous; out_nobias: the forward's output without bias and ReLU; dwork:
 *   float32 [n_nodes, heads] scratch, receives D).  Two gather launches, no floating-point atomics: the same bits on every call.
 * Domain: 1 <= heads <= 8, f % 4 == 0, f % heads == 0, (f / heads) % 4 == 0, 16-byte aligned rows (pointers and row strides) of
 * z, out, out_nobias, gout, gz and bias.  Anything else, and a null pointer, is EPS_EINVAL before any HIP call.
 * Additions: no existing call changes, EPS_ABI_VERSION stays. */
int eps_gat_aggregate(const int64_t *rowptr, const int32_t *col, int64_t row0, int64_t n_rows, int64_t n_nodes,
                      const float *z, int64_t ldz, int32_t heads, int32_t f, const float *s_src, const float *s_dst,
                      int64_t lds, float slope, const float *bias, int relu, float *out, int64_t ldo, float *lse,
                      void *stream);
int eps_gat_aggregate_backward(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, const float *z, int64_t ldz,
                               int32_t heads, int32_t f, const float *s_src, const float *s_dst, int64_t lds, float slope,
                               const float *lse, const float *out_nobias, int64_t ldo, const float *gout, int64_t ldg,
                               float *gz, int64_t ldgz, float *g_s_src, float *g_s_dst, float *dwork, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EPS_ABI_H */
