/*
 * anorag.h — C ABI of libanorag_hip.so, the MI355X (gfx950) dense-retrieval hot path of AnoRAG.
 *
 * The reference (Kevinwu901113/ano-rag) is pure Python and has no FFI of its own; its hot path leaves
 * the repo at three third-party calls.  Every entry point below replaces one of those call sites (cited
 * per function as <reference file>:<line>).  The Python classes under ano-rag_amd/ (same names as the
 * reference's: EmbeddingManager / VectorIndex / VectorRetriever / HybridSearcher) are the only callers.
 *
 * Conventions
 *   - plain C types only; row-major float32 in/out, int64 ids, every buffer caller-allocated;
 *   - every function returns 0 on success and a negative ANR_E* code on failure; the message for the
 *     calling thread's last failure is anr_last_error();
 *   - "host" pointers are ordinary process memory, "_dev" pointers are HIP device memory of the handle's
 *     device; `stream` is a hipStream_t passed as void* (NULL = the handle's own stream);
 *   - a handle serialises its own calls internally (searches on one handle may be issued from several
 *     threads: reference query/query_processor.py:2761-2766 does exactly that).
 */
#ifndef ANORAG_H
#define ANORAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANR_OK 0
#define ANR_EINVAL (-1)   /* bad argument                                   */
#define ANR_EHIP (-2)     /* a HIP runtime call failed (no device, OOM, …)  */
#define ANR_ESTATE (-3)   /* call not valid in the handle's current state   */
#define ANR_EINTERNAL (-4)

#define ANR_METRIC_IP 0 /* larger is better; cosine == IP on rows normalised at add time */
#define ANR_METRIC_L2 1 /* squared L2, smaller is better (faiss IndexFlatL2 convention)   */

const char *anr_last_error(void);
const char *anr_version(void);
/* number of visible HIP devices (0 when there is none); never fails */
int anr_device_count(void);

/* Device buffers for callers that hold no GPU runtime of their own (the Python classes pass the array sources of
 * anr_fuse_dense / the output of anr_bm25_scores_dev this way).  kind: 0 host->device, 1 device->host, 2 device->device. */
int anr_device_malloc(int32_t device, int64_t bytes, void **out);
int anr_device_free(int32_t device, void *ptr);
int anr_device_copy(int32_t device, void *dst, const void *src, int64_t bytes, int32_t kind);

/* ------------------------------------------------------------------------------------------------
 * Exact flat index: replaces faiss.IndexFlatIP / IndexFlatL2 as used by
 * vector_store/vector_index.py:77-80 (create), :187-196 (add), :223 (search), :415-426 (reset).
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_index anr_index;

/* dim: embedding dimension; metric: ANR_METRIC_*; normalize != 0 → rows and queries are L2-normalised
 * exactly as vector_index.py:265-282 does (zero-norm rows stay zero); device: HIP ordinal. */
int anr_index_create(int32_t dim, int32_t metric, int32_t normalize, int32_t device, anr_index **out);
int anr_index_destroy(anr_index *h);
/* pre-size device storage for n rows (optional; add grows geometrically otherwise) */
int anr_index_reserve(anr_index *h, int64_t n);
/* append n rows; sequential ids continue from ntotal (IndexFlat.add, vector_index.py:196) */
int anr_index_add(anr_index *h, const float *x_host, int64_t n);
int anr_index_add_dev(anr_index *h, const float *x_dev, int64_t n, void *stream);
int64_t anr_index_ntotal(const anr_index *h);
int32_t anr_index_dim(const anr_index *h);
int anr_index_reset(anr_index *h);
/* Edit the stored rows in place on the device (no corpus round trip; the row-major float32 rows are compacted or rewritten
 * and every scan image and certificate statistic is re-derived from them).  `rows` are the index's own row numbers
 * 0 .. ntotal-1 (ANR_OPT_ID_OFFSET is not applied).  Both calls retire every in-flight batch first (a batch submitted before
 * the edit answers from the pre-edit rows), return when the device work is complete, mark a graph index on the rows stale
 * and leave ANR_OPT_SCAN_BITS and the coarse image's K' ladder alone.  All device memory they need is allocated before the
 * first byte changes: an allocation failure leaves the index as it was.
 * anr_index_remove: faiss.IndexFlat.remove_ids (vector_index.py:587-608 without the rebuild) — duplicates and rows outside
 *   [0, ntotal) are ignored, *n_removed (may be NULL) counts the distinct rows dropped, survivors keep their order and are
 *   renumbered densely; removing every row leaves the state of anr_index_reset.  The largest norm and image errors are
 *   recounted over the survivors, so dropping the row that held a maximum tightens the certificate again.
 * anr_index_update: x_host[i] replaces row rows[i], preprocessed and stored bit for bit as anr_index_add would have stored
 *   it (normalised unless ANR_OPT_ADD_RAW); any row outside [0, ntotal) -> ANR_EINVAL with nothing changed; of a row listed
 *   more than once the last entry wins. */
int anr_index_remove(anr_index *h, const int64_t *rows_host, int64_t n, int64_t *n_removed);
int anr_index_update(anr_index *h, const int64_t *rows_host, const float *x_host, int64_t n);
/* copy the stored (already preprocessed) float32 rows [i0, i0+n) back to the host */
int anr_index_reconstruct(anr_index *h, int64_t i0, int64_t n, float *out_host);

/* Diagnostics of the image the streaming scan reads (what pins ANR_OPT_SCAN_BITS 12 in the tests): rows [i0, i0 + n) of the
 * f16 image (bits = 16) or of the 12-bit image (bits = 12; ANR_ESTATE when the index keeps none) decoded to float32, and the
 * statistics the certificate uses — the largest row norm and the largest ||image row - stored float32 row|| of either image
 * (max_err12 = 0 without a 12-bit image) — with the image batches currently scan (12 or 16).  Any pointer may be NULL. */
int anr_index_reconstruct_scan_image(anr_index *h, int32_t bits, int64_t i0, int64_t n, float *out_host);
int anr_index_scan_image_stats(anr_index *h, int32_t *bits_in_use, float *max_norm, float *max_err16, float *max_err12);
/* The 8-bit image (bits = 8 above, and bits_in_use 8): its largest ||image row - stored float32 row|| (0 without one). */
int anr_index_scan_image_err8(anr_index *h, float *max_err8);

/* Search nq queries for the k best rows (vector_index.py:223).  D[nq*k] scores best-first (inner
 * product, or squared L2), I[nq*k] row ids, padded with -1 (and -FLT_MAX / +FLT_MAX scores) when
 * k > ntotal, the faiss convention vector_index.py:234 relies on.  Ties in score are ordered by
 * ascending id.  Results are the exact top-k of the stored float32 rows.  k <= 1024 runs the streaming
 * pipeline; larger k (up to 2^20, synchronous calls only) computes every row's exact score and sorts on the device. */
int anr_index_search(anr_index *h, const float *q_host, int64_t nq, int32_t k, float *D, int64_t *I);
/* queries already in device memory (the output of anr_encoder_forward_dev), results to host buffers */
int anr_index_search_devq(anr_index *h, const float *q_dev, int64_t nq, int32_t k, float *D, int64_t *I);
/* same with device buffers, asynchronous on `stream` apart from one small status read-back */
int anr_index_search_dev(anr_index *h, const float *q_dev, int64_t nq, int32_t k, float *D_dev,
                         int64_t *I_dev, void *stream);

/* Asynchronous form: enqueues the search and returns.  Up to three batches are in flight (rotating workspaces), so
 * successive calls queue back to back on the device with no host synchronisation in between; `stream` is the stream the
 * queries were produced on (the batch waits for it when it is busy; NULL is the handle's own stream, NOT the legacy null
 * stream — queries produced on the null stream are handed over through a stream that waits for it, as
 * anorag_hip.sharded.ShardedStream.submit does).  D_dev / I_dev of calls still in flight must be
 * distinct buffers.  Results may be READ only after anr_index_wait() / anr_index_sync() have retired the batch: retiring
 * waits for it, runs the exact path for the queries whose certificate failed (patching D_dev / I_dev) and folds the
 * statistics.  (Until round 4 every call also made `stream` wait for the batch — ANR_OPT_STREAM_WAIT 1 restores that; the
 * marker ordered nothing that the retire does not, and in the device's four shared hardware queues it sat in front of the
 * NEXT batches' kernels: 0.348 -> 0.314 ms per batch at the 8-GPU shard size without it.) */
int anr_index_search_dev_async(anr_index *h, const float *q_dev, int64_t nq, int32_t k, float *D_dev,
                               int64_t *I_dev, void *stream);
int anr_index_sync(anr_index *h);
/* Partial form of anr_index_sync(): retires the OLDEST in-flight batches (a batch = up to 64 queries of one
 * asynchronous call) until at most `keep` (0..2) are still in flight.  The retired batches' D_dev / I_dev rows are
 * FINAL on return, while the newer ones keep the device busy — what a caller that must hand results on (the
 * row-sharded exchange of bench.py / anorag_hip/sharded.py) uses to stay pipelined without ever merging a
 * batch whose certificate recovery has not run. */
int anr_index_wait(anr_index *h, int32_t keep);

/* Exact scores of given rows: out[q][j] = score(query q, stored row ids[q][j]) — the
 * gather(note_embeddings, ids) . q that query/query_processor.py:3543-3589 recomputes per candidate
 * (there by re-encoding every candidate).  Queries are preprocessed like search queries; ids outside
 * [0, ntotal) give NaN.  Opt-in helper: the reference never takes this path. */
int anr_index_score_rows(anr_index *h, const float *q_host, int64_t nq, const int64_t *ids_host,
                         int32_t per_query, float *out_host);

/* All-pairs similarity of two sets of embeddings: EmbeddingManager.compute_similarity,
 * vector_store/embedding_manager.py:586-629, as one tiled kernel.  a [m][d], b [n][d] float32 host buffers;
 * metric 0 = cosine (rows / (||row|| + 1e-8) on both sides in float32, then the dot product, :602-609),
 * 1 = dot (:620), 2 = euclidean as 1 / (1 + ||a - b||) (:613-616).  Products are accumulated in float64;
 * out [m][n] float64 (the caller casts to the reference's result dtype). */
int anr_similarity_matrix(int32_t device, const float *a_host, int64_t m, const float *b_host, int64_t n, int32_t d,
                          int32_t metric, double *out_host);

/* Self join: every pair i < j of stored rows whose inner product reaches `threshold` — for a cosine
 * index (normalize = 1) the thresholded upper triangle of the N x N similarity matrix that
 * graph/relation_extractor.py:769-782 forms in full and :604-608 scans pair by pair, without the matrix.
 * Inner-product metric only.  Writes up to `cap` pairs (i, j, exact f32 score of the stored rows; order
 * unspecified) and sets *n_pairs to the number of qualifying pairs.  If the device-side lists were too
 * small, nothing is written, *n_pairs is set to minus an upper bound on the number of pairs, and the call
 * returns ANR_OK: call again with cap >= that bound. */
int anr_index_self_join(anr_index *h, float threshold, int64_t cap, int64_t *I_host, int64_t *J_host,
                        float *S_host, int64_t *n_pairs);

/* DBSCAN topic clustering of the stored rows: what sklearn's DBSCAN(eps, min_samples, metric).fit_predict returns in the
 * `dbscan` branch of TopicClustering._cpu_clustering (doc/clustering.py:88-99; reached from cluster_notes, :22-29, which
 * DocumentProcessor.process_documents calls on every build, doc/document_processor.py:181; the reference's GPU path,
 * utils/gpu_utils.py:123-152, is cuML and does not exist on ROCm).  Distance: Euclidean on an L2 index; on an
 * inner-product index with normalize = 1 the cosine distance 1 - x_i . x_j of the stored rows; an inner-product index
 * without normalisation is ANR_EINVAL.  A row is a core row if at least min_samples rows (itself included) lie within
 * eps of it; clusters are the connected components of the core rows under "within eps", numbered from 0 in the order of
 * their smallest core row; a row that is not core takes the smallest label among its core neighbours, or -1 (noise).
 * The decision D <= eps is the float64 one on the stored float32 rows: pairs the f16 image cannot decide are re-scored.
 * The eps pairs are consumed on the device: memory beyond the index is O(ntotal) plus the list of re-scored pairs.
 * labels_host: int32 [ntotal].  stats (8 words, may be NULL): [0] clusters, [1] core rows, [2] noise rows, [3] pairs
 * re-scored, [4] tile walks run, [5] pointer-jumping rounds, [6] times the re-score list was regrown, [7] re-scored
 * pairs found within eps.  ANR_EINVAL: eps NaN or negative, min_samples < 1.  ANR_ESTATE: a stored value is outside the
 * f16 range.  ntotal == 0: ANR_OK, nothing written. */
int anr_index_dbscan(anr_index *h, double eps, int32_t min_samples, int32_t *labels_host, int64_t *stats);

/* Diversity scheduling of fused candidates: the arithmetic of DiversityScheduler.schedule_candidates
 * (retrieval/diversity_scheduler.py:523, called from query/query_processor.py:3367) for a batch of nq queries, each with
 * a ragged candidate list offs[q] .. offs[q + 1] (offs has nq + 1 entries, offs[0] = 0).  Two steps:
 *   similarity — one C x C float64 matrix per query: the cosine of the stored float32 rows named by rows_host (row ids
 *     of the index), clamp(a_i . a_j / (||a_i|| ||a_j||), 0, 1) and 0 where a norm is zero (:431-444), whatever the index's
 *     metric or normalisation; the products are exact in float64, accumulated in one fixed order, so the value depends on
 *     the two rows alone and equal rows give equal columns.  With sim_host != NULL (the concatenated C_q x C_q blocks,
 *     float64, row-major) that matrix is taken as given instead: h may then be NULL (the call runs on `device`) and
 *     rows_host is ignored;
 *   decision — per query, on that matrix, scores_host (float64) and type_masks_host (uint32, bit t = evidence type t;
 *     NULL = no types), in the reference's float64 order of operations:
 *       dedup (:383-401; skipped when p->dedup == 0): in input order, the first kept entry with sim >= similarity_threshold
 *         either survives, or, when the new score is strictly greater, is removed and the new candidate appended;
 *       kept <= max_candidates: the kept list as it is (:655); otherwise a stable sort by score descending (:659) and
 *       p->quota == 0: the first of the sorted list, then greedily the candidate with the largest
 *         0.7 (1 - mean sim to the selected) + 0.3 min(1, score) (:666-687, :781-805);
 *       p->quota != 0: round one takes, in sorted order, every candidate with a type below its quota (:698-719); round
 *         two greedily the largest 0.5 score + 0.3 gain + 0.2 bonus, bonus as :761-779 summed over the candidate's types in
 *         ascending bit order (:724-754);
 *       a candidate wins only with a value strictly above -1.0 and strictly above every earlier one: ties go to the
 *       earlier position of the sorted list, and a step without a winner ends the selection (:684, :753).
 * Outputs (host): kept / selected: int32 [offs[nq]], query q's entries from offs[q], positions within the query's list, in
 * kept order / selection order; n_kept / n_selected: int32 [nq]; sel_sim: float64, query q's block starts at the sum of
 * min(C_r, max_candidates)^2 over r < q and holds the K x K similarities of its K selected candidates, row-major with
 * row length K (what SemanticDiversityEvaluator.evaluate_diversity, :173-194, sums).  Any output pointer may be NULL.
 * ANR_EINVAL: a list longer than 1024, a row id outside [0, ntotal), max_candidates < 1, a threshold that is NaN,
 * offs not ascending from 0, h == NULL without sim_host.  nq == 0 or all lists empty: ANR_OK. */
typedef struct anr_diversity_params {
  int32_t max_candidates;
  int32_t dedup;               /* 0: skip the dedup stage */
  int32_t quota;               /* 0: plain greedy form, else the evidence-quota form */
  int32_t reserved;
  double similarity_threshold;
  double balance_factor;       /* quota_balance_factor */
  int32_t quotas[32];          /* quota of evidence type t (0 = none) */
} anr_diversity_params;
int anr_index_diversify(anr_index *h, int32_t device, int64_t nq, const int64_t *offs, const int64_t *rows_host,
                        const double *sim_host, const double *scores_host, const uint32_t *type_masks_host,
                        const anr_diversity_params *p, int32_t *kept, int32_t *n_kept, int32_t *selected,
                        int32_t *n_selected, double *sel_sim);
/* Developer timing of anr_index_diversify (tools/diversity_perf.py; process-wide, not for concurrent callers): enable != 0
 * makes later calls record HIP events; ms3 (may be NULL) receives the last timed call's milliseconds: [0] the similarity
 * kernels (or the upload of sim_host), [1] the decision kernel, [2] first copy in to last copy out. */
int anr_diversify_timing(int32_t enable, float *ms3);

/* The second hop of the multi-hop query path for a batch of nq queries, each with a ragged candidate list
 * offs[q] .. offs[q + 1] of at most 1024 candidates (offs as in anr_index_diversify): the arithmetic of
 * QueryProcessor._rerank_khop_candidates (query/query_processor.py:1549-1635) and _apply_cluster_suppression
 * (:1637-1697), float64 in the reference's order of operations.  Host pointers in and out; any output pointer may be NULL.
 *
 * anr_index_khop_rerank.  Per candidate c: rows_host (row id of the index), bm25, is_prf (retrieval_method ==
 * "prf_bridge") and prf_sim (its similarity_score), cov and cons (_compute_cov_cons), hop_no, and decay — the factor the
 * caller prepared, hop_decay ** (hop_no - 1), or 1.0 where the reference does not multiply; the device only multiplies.
 * Per query: query_host and focus_host, float32 [nq][dim] (focus_host may be NULL), and has_focus, uint8 [nq] (NULL: no
 * query has a focus phrase).
 *   dense[c]   = max(0.0, q . x_c / (||q|| ||x_c||)) from the stored float32 row, whatever the index's metric; 0.0 where
 *                a norm is zero.  Products are exact in float64; lane l of a wave sums k = l, l + 64, ... in ascending k
 *                and the 64 sums meet in a fixed butterfly, so the value depends on the two vectors alone.
 *   focused[c] = the same with the focus vector; 0.0 for a query without a focus.
 *   With dense_host != NULL, dense_host and focused_host (float64 [offs[nq]]; focused_host NULL = all 0.0) are taken as
 *   given instead: h may then be NULL (the call runs on `device`) and rows_host and the vectors are ignored.
 *   ranks (:1590-1601): 1-based positions by score descending, ties in candidate order — one ranking by dense, one by
 *     bm25, and one by prf_sim over the candidates with is_prf only;
 *   rrf = ((0.0 + 1.0 / (rrf_k + r_dense)) + 1.0 / (rrf_k + r_bm25)), and + 1.0 / (rrf_k + r_prf) last for a PRF candidate;
 *   fw = focused_w2 when hop_no == 2, else max(0.0, focused_w2 - 0.10 * (hop_no - 2));
 *   final = ((((dense_w * dense + bm25_w * bm25) + fw * focused) + cov_w * cov) + cons_w * cons) + rrf_lambda * rrf, then
 *   final = final * decay[c];  order: the stable sort by final descending.
 * Outputs: dense, focused, final_score float64 [offs[nq]]; order int32 [offs[nq]], query q's entries from offs[q],
 * positions within the query's list, best first.
 *
 * anr_index_cluster_suppress.  cos(i, j) = G_ij / ((||x_i|| + 1e-8) (||x_j|| + 1e-8)), G the float64 Gram of the stored
 * rows (the tile of anr_index_diversify, ||x_i|| = sqrt(G_ii)); with sim_host != NULL (concatenated C_q x C_q float64
 * blocks, row-major; only j > i is read) the cosines are taken as given, h may be NULL and rows_host is ignored.  In input
 * order i: an unused i forms a cluster with every later unused j with cos(i, j) >= thr (to the seed, not transitive); the
 * cluster is stably sorted by score_host descending, its first keep_m are appended to the kept list, every member is marked
 * used; at the end the kept list is stably sorted by score descending.  The input need not be sorted.
 * Outputs: kept int32 [offs[nq]], query q's n_kept[q] entries from offs[q], positions within the query's list.
 *
 * ANR_EINVAL (nothing is written): a list longer than 1024, a row id outside [0, ntotal), keep_m < 1, a NaN in any score,
 * weight or thr, offs not ascending from 0, h == NULL while rows must be read.  nq == 0 or all lists empty: ANR_OK. */
typedef struct anr_khop_params {
  double dense_w, bm25_w, focused_w2, cov_w, cons_w, rrf_lambda, rrf_k;
} anr_khop_params;
int anr_index_khop_rerank(anr_index *h, int32_t device, int64_t nq, const int64_t *offs, const int64_t *rows_host,
                          const float *query_host, const float *focus_host, const uint8_t *has_focus,
                          const double *dense_host, const double *focused_host, const double *bm25, const uint8_t *is_prf,
                          const double *prf_sim, const double *cov, const int32_t *cons, const int32_t *hop_no,
                          const double *decay, const anr_khop_params *p, double *dense, double *focused,
                          double *final_score, int32_t *order);
int anr_index_cluster_suppress(anr_index *h, int32_t device, int64_t nq, const int64_t *offs, const int64_t *rows_host,
                               const double *sim_host, const double *score_host, double thr, int32_t keep_m, int32_t *kept,
                               int32_t *n_kept);
/* Developer timing of the two calls above (tools/khop_perf.py; process-wide, not for concurrent callers): enable != 0 makes
 * later calls record HIP events; ms6 (may be NULL) receives the last timed calls' milliseconds: rerank [0] the dot kernel,
 * [1] the rerank kernel, [2] first copy in to the last kernel; suppression [3] the Gram kernel (or the upload of sim_host),
 * [4] the suppression kernel, [5] first copy in to the last kernel. */
int anr_khop_timing(int32_t enable, float *ms6);

/* Cluster quality of a labelling of the stored rows: the two measures of TopicClustering._analyze_clusters
 * (doc/clustering.py:171-215), which cluster_notes (:20-46) runs after every clustering.  L2 index without normalisation
 * only (ANR_EINVAL otherwise): the float32 rows are used exactly as stored.  Everything comes from one float64 Gram
 * G = X X^T (f64 MFMA, float32 operands widened, one fixed k-order, squared norms from its own diagonal):
 *   silhouette (:206-213, sklearn.metrics.silhouette_samples, metric euclidean) — D_ij = sqrt(max(G_ii + G_jj - 2 G_ij, 0)),
 *     a_i the mean distance to the other rows of i's label, b_i the smallest mean distance to the rows of another label,
 *     s_i = (b_i - a_i) / max(a_i, b_i); every distinct label value is a cluster, the noise label -1 included, as in the
 *     reference's call; s_i = 0 for a label of one row, for 0 / 0, and when there is no other label.  Samples are produced
 *     for any labelling: whether the reference would report 0.0 instead (fewer than 2 clusters, or a number of distinct
 *     labels outside 2 .. ntotal - 1, where sklearn raises) is the caller's decision;
 *   cohesion (:197-203, scipy pdist cosine) — per label >= 0 with at least two rows, the mean and the population standard
 *     deviation (ddof = 0, taken against the finished mean in a second pass) of 1 - G_ij / (sqrt(G_ii) sqrt(G_jj)) over its
 *     pairs i < j, the cosine clipped to [-1, 1] as scipy does; a pair with a zero row is NaN and makes both values NaN.
 * Identical rows are at distance exactly 0.  No floating-point atomics: every output is one fixed sequence of operations, two
 * calls are bit-equal.  Memory beyond the index is O(ntotal) plus 8 bytes per 64 x 64 tile of a cluster's pairs.
 * labels_host: int32 [ntotal], any values.  Outputs (host; any pointer may be NULL): sil_samples float64 [ntotal] in row
 * order; sil_mean their mean; labels_out int32 / sizes int64 / cohesion / cohesion_std float64 [label_cap]: the distinct
 * labels ascending, their sizes and the two cohesion values (NaN where not defined: label < 0 or one row); n_labels: the number
 * of distinct labels.  stats (8 words, may be NULL): [0] distinct labels, [1] rows labelled -1, [2] 64 x 64 tiles of the
 * silhouette walk, [3] tiles of one cohesion pass, [4] clusters with a cohesion, [5] bytes of scratch held on the handle,
 * [6] MFMA steps per tile, [7] 0.  ANR_EINVAL: labels_host NULL; label_cap smaller than the number of distinct labels
 * while a per-label output is asked for (*n_labels then holds the count needed).  ntotal == 0: ANR_OK, nothing written. */
int anr_index_cluster_quality(anr_index *h, const int32_t *labels_host, double *sil_samples, double *sil_mean,
                              int64_t label_cap, int32_t *labels_out, int64_t *sizes, double *cohesion, double *cohesion_std,
                              int64_t *n_labels, int64_t *stats);
/* Developer timing of anr_index_cluster_quality (tools/cluster_quality_perf.py; process-wide, not for concurrent callers):
 * enable != 0 makes later calls record HIP events; ms3 (may be NULL) receives the last timed call's milliseconds: [0] sort,
 * norms, silhouette walk and mean, [1] the cohesion passes, [2] first copy in to last copy out. */
int anr_cluster_quality_timing(int32_t enable, float *ms3);

/* K-means topic clustering on the stored rows: sklearn's KMeans(n_clusters = k, n_init, random_state).fit as the reference
 * calls it — the `kmeans` branch of TopicClustering._cpu_clustering (doc/clustering.py:80-87), _fallback_clustering
 * (:101-108) and the fits of _find_optimal_k (:110-134).  L2 index without normalisation only (ANR_EINVAL otherwise): the
 * float32 rows are used exactly as stored.  sklearn's random draws do not depend on the data, so the caller makes them
 * (numpy RandomState, one stream for all inits) and hands them over: first_rows int64 [n_init], the first centre of every
 * init (`choice`); uniforms float64 [n_init][k - 1][n_local_trials] in [0, 1], the `uniform` draws of every further centre;
 * n_local_trials = 2 + int(ln k) in sklearn, 1 .. 8 here.
 *   seeding (sklearn _kmeans_plusplus): per step an inclusive float64 cumulative sum of the closest squared distances
 *     (Hillis-Steele inside blocks of 256, block offsets added in ascending order), searchsorted-left of u * potential
 *     clipped to ntotal - 1, distances of all rows to the candidates, one potential per candidate, the first smallest wins;
 *   Lloyd (sklearn _kmeans_single_lloyd): assignment by argmin over |x|^2 + |c|^2 - 2 x.c (f64 MFMA, ties to the lower
 *     centre), centres as per-centre sums over rows in ascending order (chunks of 512 rows, chunks in ascending order)
 *     divided by the counts; stops when no label changed, else when sum |c_new - c_old|^2 <= tol, and then assigns once more
 *     against the final centres; at most max_iter iterations (sklearn: 300); tol = tol_scale (sklearn: 1e-4) times the mean
 *     per-dimension variance of the rows, taken on the device in two passes;
 *   best of n_init: a later init replaces the best only if its inertia sum |x - c_label|^2 is strictly lower and it is not
 *     the same partition under a renaming of the labels.
 * All float64 in one fixed order, no floating-point atomics: two calls are bit-equal.  2 <= k <= 64
 * (ANR_EINVAL beyond, and for k > ntotal).  A cluster that loses all its rows ends the call with ANR_EEMPTY: sklearn
 * relocates such a centre through an argpartition whose order is not defined; nothing is written then but stats.
 * Outputs (host; all but labels may be NULL): labels int32 [ntotal]; centres float64 [k][dim]; inertia; n_iter (Lloyd
 * iterations of the winning init); best_init; stats (8 words): [0] Lloyd iterations of all inits, [1] assignment passes,
 * [2] seeding steps, [3] bytes of scratch held on the handle, [4] MFMA steps per tile, [5] the init that emptied a cluster
 * (-1: none), [6] inits that ended because no label changed, [7] the bits of the float64 tol. */
#define ANR_EEMPTY (-6)  /* anr_index_kmeans: a cluster lost all its rows */
int anr_index_kmeans(anr_index *h, int32_t k, int32_t n_init, int32_t n_local_trials, const int64_t *first_rows,
                     const double *uniforms, int32_t max_iter, double tol_scale, int32_t *labels, double *centres,
                     double *inertia, int32_t *n_iter, int32_t *best_init, int64_t *stats);

/* HDBSCAN's two O(N^2 d) passes on the stored rows: what sklearn 1.7's HDBSCAN(min_samples, metric='euclidean') computes
 * before its tree stage — the default branch of TopicClustering._cpu_clustering (doc/clustering.py:73-79).  L2 index
 * without normalisation only (ANR_EINVAL otherwise).  The distance is float64 sqrt(sum_k (x_k - y_k) * (x_k - y_k)), k
 * ascending, no fused operation, a correctly rounded root: sklearn's bit for bit.
 *   core[i]: the min_samples-th smallest distance of row i to all rows, itself included (1 <= min_samples <=
 *   HDBSCAN_MAX_MIN_SAMPLES and <= ntotal; ANR_EINVAL beyond).
 *   src / dst / w [ntotal - 1]: Prim's algorithm from row 0 over max(core[a], core[b], dist(a, b)); the row added next is
 *   the one with the smallest (value, row), so equal values go to the lowest row; edge i joins src[i], already in the tree,
 *   to dst[i].  One kernel launch per step on the handle's stream, none waits for the host.
 * ntotal >= 2 (ANR_EINVAL otherwise).  The rows must be finite: a device pass looks before either pass starts, and a NaN or
 * an infinity ends the call with ANR_EINVAL and nothing written.  The handle's lock is held for the whole call, the N - 1
 * launches and the final synchronisation included — seconds at 20 000 rows, minutes at 100 000 — and every other call on
 * the handle waits that long.  All outputs are host arrays.  stats (8 words, may be NULL): [0] Prim steps, [1] 64 x 64 tiles of the core-distance pass, [2] bytes of device
 * scratch of the call, [3] workgroup partials reduced per step, [4] / [5] microseconds of the core-distance pass and of
 * the Prim steps on the device (HIP events, created only when stats is given; 0 where they cannot be read). */
#define HDBSCAN_MAX_MIN_SAMPLES 16
int anr_index_hdbscan_mst(anr_index *h, int32_t min_samples, double *core, int64_t *src, int64_t *dst, double *w,
                          int64_t *stats);

/* HDBSCAN's tree stage, on the host (no device is touched): labels [n] (int32, -1 noise) from the n - 1 edges of a spanning
 * tree, as sklearn's HDBSCAN(min_cluster_size, cluster_selection_epsilon = eps, cluster_selection_method = 'eom',
 * allow_single_cluster = False) derives them — single linkage, condensed tree, stability, excess of mass, the epsilon
 * search, labels by ascending cluster id — with edges of equal weight kept in the order given (a stable sort), where
 * sklearn's np.argsort leaves their order open.  ANR_EINVAL for n < 2, min_cluster_size < 2, a negative eps, an edge that
 * names no row, a weight that is negative or not finite, and edges that close a cycle.  stats (8 words, may be NULL):
 * [0] clusters, [1] noise rows, [2] clusters of the condensed tree (the root included), [3] edges whose weight equals
 * their predecessor's in the sorted order, [4] true splits, [5] rows labelled through an ancestor that eps chose. */
int anr_hdbscan_labels(int64_t n, const int64_t *src, const int64_t *dst, const double *w, int32_t min_cluster_size,
                       double eps, int32_t *labels, int64_t *stats);

/* tuning / introspection */
#define ANR_OPT_FORCE_EXACT 1     /* 1: skip the f16 scan, run the dense exact path for every query  */
#define ANR_OPT_OVERFETCH 2       /* candidates kept per query before the exact re-score (0 = auto)  */
#define ANR_OPT_SAMPLE_ROWS 3     /* rows of the threshold sample (0 = auto)                          */
#define ANR_OPT_CAND_CAP 4        /* per-query candidate buffer entries                               */
#define ANR_OPT_TIMING 5          /* 1: record HIP-event time of the scan kernel in stats             */
#define ANR_OPT_ADD_RAW 6         /* 1: adds store rows as given (already normalised: reloading a saved index) */
#define ANR_OPT_STREAMS 7         /* streams the in-flight batches rotate over, 1..3 (default 3; 1 = one batch strictly after the other) */
#define ANR_OPT_ID_OFFSET 8       /* added to every returned id: the first global row of this shard (default 0) */
#define ANR_OPT_TINY 9            /* 1 (default): host-buffer searches of <= 4 queries run as ONE kernel launch (exact f32 rows / f64
                                     accumulate; completion by a word in pinned memory) where that is measured faster than the
                                     pipeline: k <= 64 and a short slice of rows per workgroup (e.g. k = 10 up to ~120 k x 768);
                                     2: wherever the path is structurally able (k <= 128, <= 1024 rows per workgroup; for tests);
                                     0: never.  Identical results either way */
#define ANR_OPT_FUSED_POST 10     /* 1 (default): candidate select + exact re-score + finalize run as ONE kernel per batch of more than
                                     4 queries (one workgroup per query); 2: for every batch; 0: always the three separate
                                     launches (identical results) */
int anr_index_set_option(anr_index *h, int32_t opt, int64_t value);

#define ANR_OPT_SHADOW 11         /* 0 (default): off; 1: a batch enqueued while another is still in flight (a pipelined caller) uses the
                                     "shadow" forms of its side kernels — threshold sample, ladder select, candidate select,
                                     re-score, finalize as workgroups of 4 waves, <= 56 registers, <= 58 KiB LDS, which are placed
                                     BESIDE the resident workgroups of the previous batch's scan instead of waiting for them
                                     (identical results); 2: every batch.  Measured slower than the wide kernels (a wave beside the
                                     scan waits ~8 us per memory round trip behind the scan's own requests): kept as an option */

#define ANR_OPT_SCHEDULE 12       /* 0 (default): one stream per in-flight batch (ANR_OPT_STREAMS of them); 1: role streams — all query
                                     preparations / threshold samples on one stream, all main scans on a second (strictly one after
                                     the other, in submission order), all select / re-score / finalize kernels on a third, two events
                                     per batch (measured 5 % slower at the 8-GPU shard size) */
#define ANR_OPT_STREAM_WAIT 13    /* 0 (default): results are read after anr_index_wait / anr_index_sync; 1: anr_index_search_dev_async
                                     also makes the caller's stream wait for the batch (the behaviour up to round 3) */
#define ANR_OPT_SCAN_BITS 14      /* the image of the corpus the streaming pass reads: 16 = the f16 image; 12 = a second image
                                     with every stored f16 rounded to its top 12 bits (6 mantissa bits), 25 % fewer bytes per
                                     row — the pass is HBM-bound, so it is that much shorter; 0 (default) = 12 for indexes of
                                     262 144 rows and more (built at the first such search), 16 below.  The certificate takes
                                     the coarser image's error norm (tracked per index like the f16 one) and K' grows from 192
                                     to 256 at k = 100: the results stay the exact top-k of the float32 rows.  A corpus whose
                                     certificates keep failing at the largest K' (near-duplicate neighbourhoods) goes back to
                                     the f16 image by itself.  Costs 1.5 bytes per stored value of device memory.  8 = int8
                                     codes with one f16 scale per row and 32 dimensions (1.0625 bytes per value, its own K'
                                     ladder from 320 at k = 100); 0 picks it from 2 097 152 rows on.  Only the image in use is
                                     built (with 0, the first search that wants it builds it) */

#define ANR_OPT_EDIT_CHUNK_ROWS 15 /* destination rows anr_index_remove compacts per step (gather into a staging buffer, write back);
                                     0 (default) = as many as a 256 MiB staging buffer holds.  Identical results for any value */

typedef struct anr_search_stats {
  int64_t n_queries;        /* queries of the last search call                                        */
  int64_t n_fallback;       /* of those, whose certificate failed (answered from the lists / by a second scan) */
  int64_t n_from_lists;     /* of those, recovered from the first scan's candidate lists (no second scan)  */
  int64_t n_dense_exact;    /* of those, answered by the dense exact path (forced, overflow, tiny index) */
  int64_t n_candidates;     /* candidates emitted by the scan, summed over queries                    */
  int64_t n_overflow;       /* queries whose candidate buffer overflowed                               */
  int64_t scan_bytes;       /* algorithmic bytes streamed by the dominant scan kernel (all launches)   */
  int32_t overfetch;        /* candidates re-scored per query                                          */
  int32_t sample_rows;
  float scan_ms;            /* HIP-event time of the main scan launches (ANR_OPT_TIMING)              */
  float total_ms;           /* HIP-event time of the whole call on the stream (ANR_OPT_TIMING)        */
} anr_search_stats;
/* statistics of the last synchronous search, or accumulated over the asynchronous searches retired since
 * anr_index_reset_stats() */
int anr_index_last_stats(anr_index *h, anr_search_stats *out);
int anr_index_reset_stats(anr_index *h);

/* Time line of the most recent batches of the scan pipeline (diagnostics; the reference has no counterpart — it is what
 * bench.py prints to explain a slow batch).  Retires every batch in flight, then copies up to max_batches records, oldest
 * first, ANR_BATCH_LOG_FIELDS int64 words each:
 *   [0] batch sequence number   [1] host clock (ns, monotonic) when its enqueue began   [2] when the enqueue returned
 *   [3] host clock when it was retired
 *   device clock (ns) at: [4] end of the query preparation  [5] end of the threshold sample  [6] end of the ladder select
 *   [7] first / [8] last workgroup of the main scan started  [9] end of the main scan  [10] end of the candidate select
 *   [11] end of the batch's last kernel
 *   [12] bit 0: shadow-sized side kernels; bits 8..: queries in the batch
 *   [13] host time (ns) the batch's recovery passes took at its retire (0: every certificate held)
 * (fused post kernel: [10] is 0).  *dev_minus_host_ns (may be NULL) receives an estimate of device clock - host clock,
 * good to a few microseconds, so that the two sets of times can be laid on one axis. */
#define ANR_BATCH_LOG_FIELDS 14
int anr_index_batch_log(anr_index *h, int64_t *out, int32_t max_batches, int32_t *n_out, int64_t *dev_minus_host_ns);

/* In-place row normalisation on host memory through the device (vector_index.py:276-280): rows with
 * zero norm are left unchanged. */
int anr_normalize_rows(float *x_host, int64_t n, int32_t d, int32_t device);

/* Merge P partial top-k lists per query (row-sharded corpus): Dp/Ip are [P][nq][k]
 * device buffers holding GLOBAL ids, -1 padded; writes the best k per query to D/I [nq][k].
 * larger_is_better selects the order.  Ties → lower id first. */
int anr_merge_topk_dev(int32_t device, const float *Dp_dev, const int64_t *Ip_dev, int32_t P, int64_t nq,
                       int32_t k, int32_t larger_is_better, float *D_dev, int64_t *I_dev, void *stream);
/* Same, with the parts d_stride floats / i_stride int64 apart instead of back to back — e.g. the receive
 * buffer of ONE all-gather whose per-rank chunk is [nq*k f32 | nq*k i64] (bench.py). */
int anr_merge_topk_strided_dev(int32_t device, const float *Dp_dev, const int64_t *Ip_dev, int64_t d_stride,
                               int64_t i_stride, int32_t P, int64_t nq, int32_t k, int32_t larger_is_better,
                               float *D_dev, int64_t *I_dev, void *stream);
/* The same merge for partial lists that already sit in host memory ([P][nq][k], e.g. written there by P
 * single-process shard searches): BASELINE.json north_star "per-shard local top-k merged on the host". */
int anr_merge_topk_host(const float *Dp, const int64_t *Ip, int32_t P, int64_t nq, int32_t k,
                        int32_t larger_is_better, float *D, int64_t *I);

/* ------------------------------------------------------------------------------------------------
 * Score fusion: the arithmetic of HybridSearcher.fuse, retrieval/hybrid_search.py:34-103, for a batch
 * of nq queries on the device (float64, bit-identical to the Python reference).
 * Each query has four (id, score) lists in the order dense, bm25, graph, path; ids are integers (the
 * caller maps note ids to integers), unique inside a list and listed in the caller's order (the order
 * matters for rrf ties, hybrid_search.py:66).  All lists are concatenated: `ids`/`scores` hold the
 * entries, `offs` is [nq][5] with the entry offset of each of the four lists of a query and its end.
 * method 0 = "linear" (max-normalised weighted sum, :83-100), 1 = "rrf" (:64-82).
 * Outputs per query, best first: out_ids [nq][pool] (-1 padded), out_final [nq][pool],
 * out_src [nq][pool][4] = the raw score of the id in each source or NaN when absent, out_count [nq].
 * A query may carry at most 4096 list entries in total.
 * ---------------------------------------------------------------------------------------------- */
int anr_fuse_lists(int32_t device, int32_t method, int64_t nq, const int64_t *ids, const double *scores,
                   const int64_t *offs, const double *weights /*[4]*/, double rrf_k, int32_t pool,
                   int64_t *out_ids, double *out_final, double *out_src, int32_t *out_count);

/* N-array form of the same fusion (BASELINE.json north_star: "fused elementwise+argk kernel"): a source may be the
 * full-corpus score vector that bm25_scores() returns (utils/bm25_search.py:286-340: one score per note, N of them,
 * zeros included) instead of a short list.  An ARRAY source is a device buffer [nq][array_len] and stands for the list
 * [(0, a[0]), (1, a[1]), ...]: every id < array_len is present (NaN marks an absent id), list order = id order.  The
 * other sources are short (id, score) lists in host memory (list_offs [nq + 1], at most 1024 entries per query in
 * all) or absent (all pointers NULL).  linear: any of the four sources may be arrays; rrf: exactly one of
 * dense / bm25 / graph (every id's exact rank among all N entries is counted in the streaming pass; no sort).
 * Outputs as anr_fuse_lists, bit-identical to it on the equivalent lists; pool <= 1024.  Ties in `final`: rrf —
 * the reference's ranks-dict insertion order; linear — lower id first (the reference iterates a set there). */
typedef struct anr_fuse_source {
  const void *array_dev;     /* device [nq][array_len], or NULL                  */
  int64_t array_len;
  int32_t array_dtype;       /* 0 = float64, 1 = float32                          */
  const int64_t *list_ids;   /* host, concatenated over the queries, or NULL      */
  const double *list_scores;
  const int64_t *list_offs;  /* host [nq + 1], or NULL                            */
  const double *array_max_dev; /* device [nq], or NULL: the maximum of each query's row of array_dev (non-NaN entries),
                                  when the producer knows it (anr_bm25_scores_dev, anr_bm25_combine_fields): linear
                                  then needs no max pass over the array.  Must be exact — it is the reference's
                                  max(scores) normaliser (hybrid_search.py:26-32) */
  /* SPARSE form of an array source (array_dev NULL, array_len = N > 0): row q is given by its explicit entries
   * (sparse_ids_dev[q][i], sparse_scores_dev[q][i]), i < sparse_count_dev[q] <= sparse_cap, in any order, ids distinct and
   * < N; every other id < N holds 0.0 (an explicit NaN marks an absent id) — what anr_bm25_sparse_dev leaves on the device
   * for a query whose postings touch a few thousand of the N notes.  Results are bit-identical to the same row handed
   * over as a dense array; the corpus-wide stream is replaced by work proportional to the entries.  At most ONE source
   * may be sparse (dense / bm25 / graph), the others are then short lists.  sparse_cap <= 8192: rows in any order (sorted
   * in LDS here); 8192 < sparse_cap <= 65536: every row of the call ASCENDING BY ID (checked on the device, ANR_EINVAL
   * otherwise) — the form anr_bm25_sparse_dev produces beyond 6144 documents. */
  const uint32_t *sparse_ids_dev;   /* device [nq][sparse_cap], or NULL */
  const double *sparse_scores_dev;  /* device [nq][sparse_cap]          */
  const int32_t *sparse_count_dev;  /* device [nq]                      */
  int64_t sparse_cap;
} anr_fuse_source;
typedef struct anr_fuse_dense_stats {
  int64_t n_queries;
  int64_t scan_bytes;        /* algorithmic bytes of the streaming pass: sum of array_len * sizeof(element) per query
                                (a sparse source: sparse_cap * 12 per query, the rows' capacity)                      */
  int64_t n_candidates;      /* ids the streaming pass kept, summed over queries                                    */
  float scan_ms;             /* HIP-event time of the streaming kernels (max pass + scan; a sparse source: sort + prep
                                + stage) over all sub-batches                                                          */
} anr_fuse_dense_stats;
int anr_fuse_dense(int32_t device, int32_t method, int64_t nq, const anr_fuse_source *sources /*[4]*/,
                   const double *weights /*[4]*/, double rrf_k, int32_t pool, int64_t *out_ids, double *out_final,
                   double *out_src, int32_t *out_count, anr_fuse_dense_stats *stats /* may be NULL */);

/* Weighted RRF over lists of ANY length (HybridSearcher.fuse, method rrf, when two or three lists are longer than
 * anr_fuse_lists holds — e.g. a dense score and a bm25 score for every note; retrieval/hybrid_search.py:60-72 ranks each
 * list by a stable descending sort).  Inputs as anr_fuse_lists (same offs layout, ids unique inside a list) with ids in
 * [0, n).  Each ranked list is sorted on the device in its own order (stable radix sort: equal scores keep their list
 * positions), the finals of all n ids are formed in the reference's order of operations and ordered by (final descending,
 * the reference's ranks-dict insertion order); ids held by no dense / bm25 / graph list are dropped.  Outputs as
 * anr_fuse_lists.  A correctness path (a handful of n-wide sorts per query): with ONE long list use anr_fuse_dense, which
 * counts the ranks it needs in a single streaming pass. */
int anr_fuse_rrf_long(int32_t device, int64_t nq, const int64_t *ids_host, const double *scores_host, const int64_t *offs_host,
                      int64_t n, const double *weights /*[4]*/, double rrf_k, int32_t pool, int64_t *out_ids,
                      double *out_final, double *out_src, int32_t *out_count);

/* Candidate-level fusion of QueryProcessor (opt-in, the reference's own call path re-encodes
 * candidates instead): the scoring loops of _hybrid_search (query/query_processor.py:3703-3760) and of
 * _enhanced_hybrid_search_v2 (:1104-1143) for nq queries at once, candidates of query q = entries [offs[q], offs[q+1]).
 *   mode 0 linear: v = a; s = b; s *= 0.1 if flags&1 (misses the must-have terms); v *= 1.2 per boost entity found
 *                  (n_ent); s *= 1.3 per boost predicate found (n_pred); score = wa*v + wb*s
 *   mode 1 rrf:    0-based ranks of stable descending sorts of a and of b; score = wa/(rrf_k+ra) + wb/(rrf_k+rb);
 *                  score *= 0.1 if flags&1
 *   mode 2 v2:     f = 1.0*a + 0.6*b; f *= mult[0] (section); f *= mult[1] (lexical); if f < noise and flags&1 (must-have
 *                  terms NOT satisfied): f = 0; f *= mult[2] (entity boost); f *= mult[3] (predicate boost)
 * score[] per candidate (float64, the reference's order of operations) and order[] = the candidate indices of each
 * query (relative to its range) in the stable descending order the reference sorts into.  All arrays host memory;
 * flags / n_ent / n_pred may be NULL (= 0), mult is [total][4] and required for mode 2. */
int anr_fuse_candidates(int32_t device, int32_t mode, int64_t nq, const int64_t *offs, const double *a, const double *b,
                        const int32_t *flags, const int32_t *n_ent, const int32_t *n_pred, const double *mult,
                        double wa, double wb, double rrf_k, double noise, double *score, int32_t *order);

/* ------------------------------------------------------------------------------------------------
 * Sentence encoder: replaces SentenceTransformer.encode as called at
 * vector_store/embedding_manager.py:392-399 (and :357) — transformer forward + pooling + optional L2
 * normalisation for BERT-family models (bert / roberta / xlm-roberta / mpnet).  Tokenisation is host work.
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_encoder anr_encoder;
typedef struct anr_encoder_config {
  int32_t n_layers, hidden, n_heads, intermediate;
  int32_t vocab_size, max_positions, type_vocab_size;
  int32_t pos_offset; /* 0 for bert; padding_idx + 1 (= 2) for roberta / xlm-roberta position ids          */
  int32_t pooling;    /* 0 = mean over the attention mask, 1 = CLS token (sentence-transformers Pooling)    */
  int32_t act;        /* 0 = gelu (erf)                                                                      */
  float ln_eps;
} anr_encoder_config;

int anr_encoder_create(const anr_encoder_config *cfg, int32_t device, anr_encoder **out);
int anr_encoder_destroy(anr_encoder *e);
/* Upload one float32 tensor by name (row-major, nn.Linear weights as [out][in]):
 *   emb.word emb.pos emb.type emb.ln.g emb.ln.b
 *   L<i>.{q,k,v,o,ffn1,ffn2}.{w,b}   L<i>.ln1.{g,b} (after attention)   L<i>.ln2.{g,b} (after the FFN)
 *   rel.bias (optional, MPNet): [n_heads][2 P - 1], P = max_positions - pos_offset — added to the scaled
 *   attention score of (query i, key j) at index j - i + P - 1 (all-mpnet-base-v2, the reference's second
 *   fallback model, embedding_manager.py:218-219) */
int anr_encoder_set_tensor(anr_encoder *e, const char *name, const float *data, int64_t n_elements);
int anr_encoder_finalize(anr_encoder *e); /* fails if a tensor is missing */
/* ids [B][L] (right-padded), lengths [B] = number of real tokens per row (the attention mask), type_ids
 * [B][L] or NULL; out_host [B][hidden] float32.  normalize != 0 applies F.normalize(p=2, dim=1). */
int anr_encoder_forward(anr_encoder *e, const int32_t *ids, const int32_t *lengths, const int32_t *type_ids,
                        int32_t B, int32_t L, int32_t normalize, float *out_host);

/* The same forward with the embeddings left in DEVICE memory (caller-allocated on the encoder's device, float32
 * rows of `hidden`): sequence b goes to row out_rows[b] (host array [B]; NULL = row b), so the length-sorted batches
 * of SentenceTransformer.encode land in input order.  Feeds anr_index_add_dev / anr_index_search_dev directly — the
 * index build (vector_store/retriever.py:140-157) and the query path (:206-216) without the device -> host -> device
 * round trip per batch.  out_dev is complete when the call returns. */
int anr_encoder_forward_dev(anr_encoder *e, const int32_t *ids, const int32_t *lengths, const int32_t *type_ids,
                            int32_t B, int32_t L, int32_t normalize, float *out_dev, const int32_t *out_rows);
/* anr_encoder_forward for callers that share the handle from several threads with a query or a few each (the reference's
 * query-time pattern: main_musique.py:487-494, query/query_processor.py:2761-2766): calls that arrive while a forward is
 * running wait in a combining queue and are merged into the next forward — same normalize flag, same use of type_ids, at most
 * 2048 padded tokens per forward, so an embedding never depends on who else was in flight: bit-identical to
 * anr_encoder_forward.  Larger requests run alone, as anr_encoder_forward.  anr_encoder_shared_stats: forwards run and
 * requests served through the queue so far (either pointer may be NULL). */
int anr_encoder_forward_shared(anr_encoder *e, const int32_t *ids, const int32_t *lengths, const int32_t *type_ids,
                               int32_t B, int32_t L, int32_t normalize, float *out_host);
int anr_encoder_shared_stats(anr_encoder *e, int64_t *forwards, int64_t *requests);

/* ------------------------------------------------------------------------------------------------
 * BM25 scoring: SimpleBM25.get_scores / bm25_scores of utils/bm25_search.py:43-63,
 * :286-340 over a CSR postings image.  Tokenisation, term ids and the float64 posting weights
 *   w(t,d) = idf_t * (tf*(k1+1) / (tf + k1*(1 - b + b*(dl_d/avgdl))))
 * are host work (anorag_hip/bm25_search.py); the device adds them per query in the reference's order, so the
 * float64 scores are bit-identical.  normalize != 0 divides by the maximum when it is > 0 (:329-333).
 * A term's posting list holds each document once, document ids strictly ascending (checked at create).
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_bm25 anr_bm25;
int anr_bm25_create(int32_t device, int64_t n_docs, int64_t n_terms, const int64_t *indptr /*[n_terms+1]*/,
                    const int32_t *doc_ids, const double *weights, anr_bm25 **out);
int anr_bm25_destroy(anr_bm25 *h);
/* query i = term ids q_terms[q_indptr[i] .. q_indptr[i+1]) in query-token order (repeats count twice, unknown
 * tokens are simply omitted).  out_host: dense [nq][n_docs] float64. */
int anr_bm25_scores(anr_bm25 *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, int32_t normalize,
                    double *out_host);
/* the same scores left in DEVICE memory ([nq][n_docs] float64, caller-allocated on the handle's device): the array
 * source anr_fuse_dense takes — the N-vector never crosses PCIe.  max_dev (device [nq], may be NULL): the maximum of each
 * output row, a by-product of the scoring (a pass over the query's postings, not over n_docs) — hand it to
 * anr_fuse_source.array_max_dev and linear fusion needs no max pass of its own */
int anr_bm25_scores_dev(anr_bm25 *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, int32_t normalize,
                        double *out_dev, double *max_dev);
/* FieldWeightedBM25 (utils/bm25_search.py:66-146, :190-234): per field one anr_bm25 handle scores the queries
 * (anr_bm25_scores_dev, normalize = 0); this adds the fields up — total = sum_f weights[f] * field_scores[f], in field
 * order, float64, bit-identical to get_scores — and, with normalize != 0, divides by the per-query maximum when it is
 * > 0 (field_weighted_bm25_scores).  field_scores_dev: host array of n_fields (<= 8) device pointers [nq][n_docs];
 * out_dev [nq][n_docs] on the same device (it may be one of the inputs); max_dev as in anr_bm25_scores_dev. */
int anr_bm25_combine_fields(int32_t device, int32_t n_fields, const double *const *field_scores_dev,
                            const double *weights, int64_t nq, int64_t n_docs, int32_t normalize, double *out_dev,
                            double *max_dev);
/* The scores of anr_bm25_scores_dev in SPARSE form, left on the device for anr_fuse_dense (anr_fuse_source.sparse_*): per
 * query the documents its postings touch — ids_dev / scores_dev [nq][cap] (cap <= 65536), count_dev [nq], max_dev
 * [nq] (may be NULL; the maximum over all n_docs scores, the untouched zeros included).  The N-vector is never
 * materialised.  cap <= 6144: a workgroup accumulates its query in an LDS hash table, rows unordered; 6144 < cap <= 65536
 * (round 4): the row is cut into slices of the document range, one workgroup per slice (presence bits -> rank = slot, sums
 * in LDS), rows ASCENDING BY ID — what anr_fuse_dense asks of rows beyond 8192 entries.  Either way a document's additions
 * happen one at a time in the reference's token order, so every score equals anr_bm25_scores' bit for bit.  A query that
 * touches more than cap documents gets count -1 (its row is unusable: score that query with anr_bm25_scores_dev); so does
 * (cap > 6144) one whose summed posting lengths exceed 4 cap or one slice of which holds more than 4096 documents.
 * out_count_host (may be NULL): the counts, copied back. */
int anr_bm25_sparse_dev(anr_bm25 *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, int32_t normalize,
                        int32_t cap, uint32_t *ids_dev, double *scores_dev, int32_t *count_dev, double *max_dev,
                        int32_t *out_count_host);
/* sparse form for the fusion: the documents with a non-zero score, unordered; out_count may exceed cap
 * (the lists are then truncated) */
int anr_bm25_nonzero(anr_bm25 *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, int32_t normalize,
                     int32_t cap, int32_t *out_docs, double *out_scores, int32_t *out_count);

/* ------------------------------------------------------------------------------------------------
 * IVF-Flat index (opt-in; replaces faiss.IndexIVFFlat where vector_index.py:81-95 builds one, :109-166 trains it and
 * :428-470 sweeps nprobe).  Separate from anr_index: nothing of the exact index changes.  Rows are assigned to the
 * nearest of nlist centroids and kept list by list; a search scores the nprobe lists nearest to each query.  Results
 * are the exact top-k of the probed lists' float32 rows (float64 re-score, ties by ascending id), padded with id -1 and
 * -FLT_MAX (IP) / +FLT_MAX (L2) when the probed lists hold fewer than k rows.  Ids are global insertion numbers and
 * survive anr_ivf_remove (faiss IVF semantics); they are never reused.  Limits: dim even and <= 2048, nlist <= 8192,
 * k <= 1024, fewer than 2^31 - 32 * nlist rows ever added.  Rows are kept twice in float32 and once in f16, and removed
 * rows keep their float32 copy until the handle is destroyed.  Training, list layout and the certificate are described at the top of csrc/ivf.hip.
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_ivf anr_ivf;

int anr_ivf_create(int32_t dim, int32_t metric, int32_t normalize, int32_t nlist, int32_t device, anr_ivf **out);
int anr_ivf_destroy(anr_ivf *h);
/* Lloyd's k-means on the device: at most 256 * nlist of the n rows (chosen by seed), initial centroids nlist distinct
 * rows chosen by seed, niter iterations; an empty list takes half of the largest one.  Deterministic: the same rows and
 * seed give bit-identical centroids.  Rows already in the index are re-assigned. */
int anr_ivf_train(anr_ivf *h, const float *x_host, int64_t n, int32_t niter, int64_t seed);
/* niter Lloyd iterations over all n rows, starting from the current centroids (anr_ivf_set_centroids) */
int anr_ivf_train_from_centroids(anr_ivf *h, const float *x_host, int64_t n, int32_t niter);
/* nlist x dim float32 centroids in / out (save and load; set re-assigns the rows already in the index) */
int anr_ivf_set_centroids(anr_ivf *h, const float *c_host);
int anr_ivf_get_centroids(anr_ivf *h, float *c_host);
int anr_ivf_is_trained(const anr_ivf *h);
/* append n rows (ids continue from the number of rows ever added); needs centroids */
int anr_ivf_add(anr_ivf *h, const float *x_host, int64_t n);
int anr_ivf_add_dev(anr_ivf *h, const float *x_dev, int64_t n);
/* raw != 0: later adds store rows as given (already normalised: reloading a saved index); queries are still normalised */
int anr_ivf_set_add_raw(anr_ivf *h, int32_t raw);
/* nq queries, the nprobe nearest lists each (nprobe > nlist means nlist): D[nq*k], I[nq*k] on the host */
int anr_ivf_search(anr_ivf *h, const float *q_host, int64_t nq, int32_t k, int32_t nprobe, float *D, int64_t *I);
int anr_ivf_search_devq(anr_ivf *h, const float *q_dev, int64_t nq, int32_t k, int32_t nprobe, float *D, int64_t *I);
/* rows in the index (removed ones excluded) */
int64_t anr_ivf_ntotal(const anr_ivf *h);
/* rows per list, nlist entries */
int anr_ivf_list_sizes(anr_ivf *h, int64_t *sizes);
/* the stored (preprocessed) float32 rows of n global ids; ANR_EINVAL for an id not in the index */
int anr_ivf_reconstruct(anr_ivf *h, const int64_t *ids, int64_t n, float *out_host);
/* drop the rows with these ids (unknown ids are ignored); the others keep their ids, the centroids stay */
int anr_ivf_remove(anr_ivf *h, const int64_t *ids, int64_t n, int64_t *n_removed);
/* 1: spherical k-means — centroids are normalised after every update of anr_ivf_train* (default 0) */
int anr_ivf_set_spherical(anr_ivf *h, int32_t on);
/* the list each of n global ids is assigned to; ANR_EINVAL for an id not in the index */
int anr_ivf_assignments(anr_ivf *h, const int64_t *ids, int64_t n, int32_t *lists);
/* of the last search: queries, and queries whose certificate failed and that were re-scored exactly over their probed rows */
int anr_ivf_last_search_stats(anr_ivf *h, int64_t *n_queries, int64_t *n_exact_rescan);
/* device and host bytes of the handle's persistent storage (rows, codes, ids, lists, centroids, codebooks; per-search
 * and per-add scratch excluded), after the list-ordered copy is brought up to date; either pointer may be NULL */
int anr_ivf_memory(anr_ivf *h, int64_t *device_bytes, int64_t *host_bytes);

/* ------------------------------------------------------------------------------------------------
 * IVF-PQ mode of the same handle (opt-in; replaces faiss.IndexIVFPQ(quantizer, d, nlist, m, 8), vector_index.py:88-92).
 * Every anr_ivf_* entry above works on it; what changes:
 *  - the coarse quantiser is IVF-Flat's.  A row is stored as its list and m one-byte codes: code j is the nearest
 *    (float64 argmin of |r_j - cb_j[c]|^2, ties to the lower code) of the 256 entries of codebook j to sub-vector j of
 *    the residual r = x - c_list (float32).  The device holds only the codes (list-ordered, m bytes per row in 64-row
 *    tiles), the ids, the list offsets, the centroids and the codebooks; the preprocessed float32 rows stay in host
 *    memory in insertion order (reconstruct, saving, re-encoding after a change of centroids or codebooks).
 *  - anr_ivf_train trains the coarse quantiser as for IVF-Flat, then the codebooks: the first min(n, 65536) rows of the
 *    same seeded permutation, their residuals, one L2 k-means of 25 iterations per sub-space (never spherical),
 *    starting from the sub-vectors of the first 256 of those rows; means and the empty-entry rule are the coarse
 *    quantiser's, so the same rows and seed give bit-identical codebooks.  Fewer than 256 rows: ANR_EINVAL.
 *  - anr_ivf_search returns the ADC top-k of the probed lists (faiss's IVFPQ answer; no re-rank against the rows), by
 *    (key desc, id asc).  IP key q.c_list + sum_j q_j.cb_j[code_j]; L2 distance sum_j |(q - c_list)_j - cb_j[code_j]|^2;
 *    the sums are float32.  D is the key (IP) or the distance (L2).  n_exact_rescan is always 0.
 * Limits: nbits == 8, m <= 128, dim % m == 0 with dim / m even, and the IVF-Flat limits.  Violations: ANR_EINVAL.
 * ---------------------------------------------------------------------------------------------- */
int anr_ivf_create_pq(int32_t dim, int32_t metric, int32_t normalize, int32_t nlist, int32_t m, int32_t nbits,
                      int32_t device, anr_ivf **out);
/* m x 256 x (dim / m) float32 codebooks in / out; set re-encodes the rows already in the index */
int anr_ivf_get_codebooks(anr_ivf *h, float *cb_host);
int anr_ivf_set_codebooks(anr_ivf *h, const float *cb_host);
/* niter Lloyd iterations of every sub-space over the residuals of all n rows, starting from the current codebooks
 * (needs centroids and codebooks); the rows in the index are re-encoded */
int anr_ivf_pq_train_from_codebooks(anr_ivf *h, const float *x_host, int64_t n, int32_t niter);
/* the list and the m code bytes (codes_out[n][m]) of n global ids; ANR_EINVAL for an id not in the index */
int anr_ivf_codes(anr_ivf *h, const int64_t *ids, int64_t n, int32_t *lists_out, uint8_t *codes_out);
/* c_list + the codebook entries of each id's codes, float32 (faiss's IVFPQ reconstruct) */
int anr_ivf_decode(anr_ivf *h, const int64_t *ids, int64_t n, float *out_host);

/* ------------------------------------------------------------------------------------------------
 * Graph index on an anr_index handle (opt-in; replaces the faiss.IndexHNSWFlat(d, 32, metric) with efConstruction 200 /
 * efSearch 100 that vector_index.py:94-99 builds): one level, fixed out-degree R, built from the handle's own exact
 * kNN lists, searched by a beam of ef entries.  The graph reads the handle's stored float32 rows (no second copy) and
 * keeps an int8 traversal image (dim rounded up to 16 bytes + 8 bytes per row) and the [n][R] int32 adjacency on the
 * device.  An add or a reset marks the graph stale: the next graph call that needs it rebuilds it with the same R and
 * build_degree (counted in builds).  Build, prune rule and search: top of csrc/graph.hip and DESIGN.md §5d.  Graph calls
 * must not overlap an add or a reset of the same handle from another thread (a build reads the rows in place).
 * Limits: dim <= 2048, fewer than 2^31 - 1 rows, R even in 2..128, build_degree in 1..255, 1 <= k, ef and
 * max(k, ef) <= 256.  Violations: ANR_EINVAL; a graph call other than build / set before any graph: ANR_ESTATE.
 * ---------------------------------------------------------------------------------------------- */
/* build the graph of the current rows (vector_index.py:94-99): exact top-(build_degree + 1) lists, pruned to R.
 * keep_knn != 0 keeps the pre-prune lists of this build and its rebuilds for anr_index_graph_knn (n * build_degree int32
 * of host memory; tests) */
int anr_index_graph_build(anr_index *h, int32_t R, int32_t build_degree, int32_t keep_knn);
/* beam search of nq queries (vector_index.py:223 on an HNSW index, efSearch = ef): D / I [nq][k] host buffers, the best
 * k rows of the beam by float64 re-score from the stored rows, ties by ascending id, padded as anr_index_search */
int anr_index_graph_search(anr_index *h, const float *q_host, int64_t nq, int32_t k, int32_t ef, float *D, int64_t *I);
int anr_index_graph_search_devq(anr_index *h, const float *q_dev, int64_t nq, int32_t k, int32_t ef, float *D,
                                int64_t *I);
/* the adjacency [n][R] (-1 padded) out / in (persistence, vector_index.py:94-99 save / load).  get rebuilds a stale
 * graph first, then needs the caller's buffer shape n, R to be the graph's (ANR_EINVAL otherwise); set needs n == ntotal */
int anr_index_graph_get(anr_index *h, int32_t *adj, int64_t n, int32_t R);
int anr_index_graph_set(anr_index *h, const int32_t *adj, int64_t n, int32_t R);
/* the pre-prune kNN lists [n][build_degree] of the last build (tests).  A stale graph is rebuilt first; the buffer
 * shape n, build_degree must be the current one (ANR_EINVAL otherwise); ANR_ESTATE when the lists were not kept
 * (built without keep_knn, or the graph came from anr_index_graph_set) */
int anr_index_graph_knn(anr_index *h, int32_t *lists, int64_t n, int32_t K);
/* rows of the traversal image decoded to float32, out [n][dim] (tests) */
int anr_index_graph_image(anr_index *h, const int64_t *ids, int64_t n, float *out);
typedef struct anr_graph_stats {
  int64_t builds;            /* graph builds so far (anr_index_graph_build and rebuilds of a stale graph) */
  int64_t last_nq;           /* queries of the last graph search                                           */
  int64_t last_iterations;   /* beam iterations (p parents expanded each), summed over those queries        */
  int64_t last_rows_scored;  /* traversal-image rows scored, summed over those queries                      */
  int64_t last_capped;       /* queries that stopped at the iteration cap instead of a fully expanded beam  */
  int64_t graph_bytes;       /* device bytes of the adjacency                                               */
  int64_t image_bytes;       /* device bytes of the traversal image                                         */
  int32_t R, build_degree;
  int32_t has_graph, stale;
  float knn_ms, prune_ms, image_ms;  /* host wall time of the phases of the last build                   */
} anr_graph_stats;
int anr_index_graph_stats(anr_index *h, anr_graph_stats *out);

/* ------------------------------------------------------------------------------------------------
 * Note graph (opt-in): the `graph` source of HybridSearcher.fuse — GraphIndex.build_index's weighted PageRank
 * (graph/graph_index.py:43-49) and GraphRetriever.retrieve's bounded shortest-path expansion from seed notes
 * (graph/graph_retriever.py:61-92), float64 throughout, on an undirected weighted graph kept as a symmetric CSR on the
 * device (int64 row offsets, int32 neighbour, float64 weight, neighbours ascending inside a row).  Unrelated to the
 * anr_index_graph_* vector index above.  Layouts, summation orders and the workspace rule: DESIGN.md §5e and the top of
 * csrc/notegraph.hip.  Calls on one handle are serialised.
 * Out of scope: the reference's fallbacks for graphs networkx cannot weigh (unweighted PageRank, graph_index.py:47-49;
 * hop-count BFS, graph_retriever.py:75-77) — such graphs are rejected at create instead; directed graphs; personalised
 * PageRank; the reasoning-path search.
 * ---------------------------------------------------------------------------------------------- */
#define ANR_ENOCONV (-5)  /* anr_notegraph_pagerank: no convergence within max_iter (networkx raises
                             PowerIterationFailedConvergence there) */
typedef struct anr_notegraph anr_notegraph;
/* the nx.Graph the reference builds (graph/graph_builder.py:21-35) as its n_edges undirected edges: distinct unordered
 * pairs (src[e], dst[e]) with ids in [0, n_nodes) (the caller maps note ids to node indices, graph_index.py:28-35) and
 * weight w[e].  ANR_EINVAL for a self-loop, a pair given twice (in either direction), a negative or non-finite weight, an
 * id out of range; n_nodes < 2^31 - 1, n_edges <= 2^30. */
int anr_notegraph_create(int32_t device, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *dst,
                         const double *w, anr_notegraph **out);
int anr_notegraph_destroy(anr_notegraph *h);
/* nx.pagerank(graph, weight="weight") of graph_index.py:46 (networkx 3.x _pagerank_scipy, uniform personalisation and
 * dangling weights, start 1/n): x <- alpha * (x A + sum_dangling(x) * p) + (1 - alpha) * p with A[i][j] = (1 / S_i) * w_ij,
 * S_i the sum of row i in ascending j, dangling = the rows with S_i == 0, until the L1 change is < n * tol.  Pull form:
 * x_new[j] adds x[i] * A[i][j] over row j in ascending i, one thread per row; the dangling sum and the L1 change are
 * fixed-shape tree sums (no float atomics, no multiply-add contraction), so the result is the same bits on every run.
 * The result becomes the handle's centrality and, when out_host is not NULL, is copied to out_host [n].  *iters (may be
 * NULL): iterations made.  ANR_ENOCONV after max_iter iterations without convergence (the handle's centrality is then
 * left as it was). */
int anr_notegraph_pagerank(anr_notegraph *h, double alpha, int32_t max_iter, double tol, double *out_host, int32_t *iters);
/* the centrality graph_retriever.py:84 looks up (GraphIndex.get_centrality), [n] float64: supplied from elsewhere / read
 * back.  Zero until a PageRank or a set. */
int anr_notegraph_set_centrality(anr_notegraph *h, const double *c_host);
int anr_notegraph_get_centrality(anr_notegraph *h, double *c_host);
/* the nodes' importance_score (graph_retriever.py:86), [n] float64; 1.0 per node until set */
int anr_notegraph_set_importance(anr_notegraph *h, const double *imp_host);
/* GraphRetriever.retrieve (graph_retriever.py:66-90) for nq seed lists at once: query q has the seeds
 * seeds[seed_offs[q] .. seed_offs[q+1]) in list order; a seed < 0 or >= n is skipped (:69-70).  Per seed one bounded
 * single-source shortest-path search (:72-74, cutoff = k_hop is a DISTANCE): label-correcting relaxations
 * d[v] = min(d[v], d[u] + w) from nodes with d[u] <= cutoff, candidates > cutoff dropped — the fixed point is Dijkstra's
 * distance bit for bit.  A node is reported once per query, with the distance from the first seed in list order that
 * reaches it; a search never reports its own seed and does not mark it visited (:79-81).
 * graph_score = (centrality / (dist + 1e-5)) * importance (:87), three float64 operations in that order.
 * Per query, best first by (score descending, seed position ascending, dist ascending, id ascending): out_ids /
 * out_dist / out_score / out_seed_pos [nq][cap], padded with -1 / NaN / NaN / -1; out_count[q] = the nodes found, which
 * may exceed cap (the best cap are kept).  out_dist, out_score, out_seed_pos may be NULL. */
int anr_notegraph_retrieve(anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds, double cutoff,
                           int32_t cap, int64_t *out_ids, double *out_dist, double *out_score, int32_t *out_seed_pos,
                           int32_t *out_count);
/* the same result left on the handle's device as rows ASCENDING BY ID: ids_dev uint32 [nq][cap], scores_dev float64
 * [nq][cap] (graph_score), count_dev int32 [nq] = min(found, cap) — the layout of anr_fuse_source.sparse_* (cap <= 65536).
 * out_found_host (may be NULL): the nodes found per query, before the cap. */
int anr_notegraph_retrieve_dev(anr_notegraph *h, int64_t nq, const int64_t *seed_offs, const int64_t *seeds,
                               double cutoff, int32_t cap, uint32_t *ids_dev, double *scores_dev, int32_t *count_dev,
                               int32_t *out_found_host);
/* Hand-off to anr_fuse_dense as its `graph` source.  The sparse form cannot carry these rows as they are: there every id
 * that is not listed holds 0.0 and is therefore PRESENT, while a note the expansion did not reach must be ABSENT from
 * `graph` (hybrid_search.py tags a result's sources by membership, and an id that only `graph` lists with 0.0 would become
 * a candidate).  Of the two ways round it — (a) a dense [nq][n] float64 array with NaN for the absent ids, (b) a short host
 * list — this is (a): a list is limited to 1024 entries per query and one seed already reaches thousands of notes, and
 * the array stays on the device.  Fills out_dev [nq][n] (caller-allocated on the handle's device) with NaN and scatters
 * the rows of anr_notegraph_retrieve_dev into it: hand it over as anr_fuse_source.array_dev with array_len = n.  Cost:
 * 8 n bytes written per query, and the fusion streams them again. */
int anr_notegraph_rows_to_array_dev(anr_notegraph *h, int64_t nq, int32_t cap, const uint32_t *ids_dev,
                                    const double *scores_dev, const int32_t *count_dev, double *out_dev);
/* options: 1 = ANR_NOTEGRAPH_OPT_MAX_SLOTS — an upper bound on the (query, seed) searches in flight at a time (0 = sized
 * from free device memory; tests force 1 to walk the sub-batching).  Results never depend on it. */
#define ANR_NOTEGRAPH_OPT_MAX_SLOTS 1
/* 2 = ANR_NOTEGRAPH_OPT_BFS_WORDS — the 64-bit words per node and pass of anr_notegraph_hop_histogram: 1, 2, 4, 8 or 16
 * (0 = the default, 16); a pass walks 64 * words sources.  Tests force 1 and 2 to walk many passes on small graphs.
 * Results never depend on it. */
#define ANR_NOTEGRAPH_OPT_BFS_WORDS 2
int anr_notegraph_set_option(anr_notegraph *h, int32_t option, int64_t value);

/* Graph quality (opt-in): the integers behind compute_metrics (graph/graph_quality.py:5-46), which
 * GraphBuilder.build_graph_with_metrics runs on every graph (graph/graph_builder.py:39-49).  Hop counts on the handle's
 * symmetric CSR; the weights are not read (nx.average_shortest_path_length is called with weight=None).  Layout, the words
 * per pass and the bytes per level: DESIGN.md §5i.
 *
 * nx.connected_components (graph_quality.py:33,37): labels_host[v] = the smallest node index of v's component, found by
 * integer atomicMin hooking and pointer jumping until a round changes nothing; *n_components (may be NULL) = the number
 * of distinct labels.  Ascending label is the order in which networkx yields the components (by first node). */
int anr_notegraph_components(anr_notegraph *h, int32_t *labels_host /*[n]*/, int64_t *n_components);
/* The sum nx.average_shortest_path_length forms (graph_quality.py:40), kept apart by hop count: counts_host[l] = the
 * number of (source, node) pairs at hop distance l, over the n_sources nodes sources[] (NULL = all n nodes, n_sources is
 * then ignored); counts_host[0] = n_sources; a pair in different components is counted nowhere.  A multi-source
 * bit-parallel BFS: 64 * words sources per pass, one pull over the CSR per level, integer popcounts added per workgroup.
 * *n_levels = the entries in use (the largest distance + 1); counts_host has room for cap entries and is zero beyond
 * *n_levels.  ANR_EINVAL for a source outside [0, n), and when more than cap levels are needed — *n_levels is then the
 * number needed and counts_host is left alone; cap = n always suffices.
 * stats8 (may be NULL), int64 [8]: 0 sources per pass, 1 passes, 2 levels walked over all passes (one launch each,
 * the closing empty level of a pass included), 3 scratch bytes in use, 4 words per node, 5 sources, 6 microseconds between two HIP
 * events around the call's work on the handle's stream (the host's reading of each level's count lies inside), 7 zero. */
int anr_notegraph_hop_histogram(anr_notegraph *h, int64_t n_sources, const int64_t *sources, int64_t cap,
                                int64_t *counts_host, int64_t *n_levels, int64_t *stats8);

/* ------------------------------------------------------------------------------------------------
 * Set-overlap join (opt-in): the two integer O(N^2) passes of RelationExtractor._extract_basic_relations
 * (graph/relation_extractor.py:104-147).  A handle holds one family of sets on one device: the rows are notes, the items
 * integer ids of entities or keywords, kept as a CSR and as its transpose (the postings).  No floating point: every output
 * is an integer and the reference's last division stays with the caller.  Layout, the LDS table, the overflow rule and the
 * cost per row: DESIGN.md §5k and the top of csrc/setjoin.hip.  Calls on one handle are serialised.
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_setjoin anr_setjoin;
/* note_to_entities / entity_to_notes of relation_extractor.py:423-432: row r holds items[indptr[r] .. indptr[r+1]), STRICTLY
 * ASCENDING ids in [0, n_items).  ANR_EINVAL, before any device work, for a row that descends or repeats an id, an id out of
 * range, indptr not ascending from 0, a row of more than 2^20 items, n_rows or n_items or indptr[n_rows] >= 2^31 - 1.  The
 * postings (item -> ascending rows) are built on the device by one stable radix sort of item << 32 | row.  Empty rows and
 * n_rows == 0 are legal. */
int anr_setjoin_create(int64_t n_rows, int64_t n_items, const int64_t *indptr, const int32_t *items, int32_t device,
                       anr_setjoin **out);
int anr_setjoin_destroy(anr_setjoin *h);
/* The pair search of extract_entity_coexistence_relations (relation_extractor.py:434-463): every pair i < j with
 * |S_i & S_j| >= min_common (min_common >= 1, ANR_EINVAL otherwise).  The result stays on the handle until the next call;
 * *n_pairs and *n_common (may be NULL) = the pairs and the shared items over all of them.  A result that does not fit in
 * the device's free memory is ANR_EHIP with the sizes in the message, never a truncation.
 * stats8 (may be NULL), int64 [8]: 0 rows that had candidates to look at, 1 candidate insertions into the table, 2 pairs kept,
 * 3 shared ids written, 4 rows_overflowed (rows that needed more than one pass of the table), 5 table slots, 6 passes summed
 * over the rows, 7 scratch bytes besides the result. */
int anr_setjoin_cooccur(anr_setjoin *h, int32_t min_common, int64_t *n_pairs, int64_t *n_common, int64_t *stats8);
/* the pairs sorted by (i, j): I, J, inter = |S_i & S_j|, uni = |S_i| + |S_j| - inter (what :476 divides by), and the shared
 * ids of pair p ascending in common_items[common_ptr[p] .. common_ptr[p+1]) (:460).  ANR_ESTATE before a cooccur call. */
int anr_setjoin_cooccur_fetch(anr_setjoin *h, int32_t *I /*[n_pairs]*/, int32_t *J, int32_t *inter, int32_t *uni,
                              int64_t *common_ptr /*[n_pairs+1]*/, int32_t *common_items /*[n_common]*/);
/* the two set sizes of _calculate_note_topic_similarity (relation_extractor.py:752-753, :761-762) for n explicit row pairs:
 * inter[p] = |S_I[p] & S_J[p]|, uni[p] = |S_I[p] | S_J[p]|.  i == j, empty rows and n == 0 are legal; a row outside
 * [0, n_rows) is ANR_EINVAL.  Does not touch the cooccur result. */
int anr_setjoin_pair_counts(anr_setjoin *h, int64_t n, const int32_t *I, const int32_t *J, int32_t *inter, int32_t *uni);
/* option 1 = ANR_SETJOIN_OPT_TABLE_SLOTS — the slots of the LDS table a workgroup of anr_setjoin_cooccur accumulates a row's
 * candidates in: a power of two in [64, 4096] (0 = the default, 4096).  Tests force 64 to walk the overflow passes on small
 * inputs.  Results never depend on it. */
#define ANR_SETJOIN_OPT_TABLE_SLOTS 1
int anr_setjoin_set_option(anr_setjoin *h, int32_t option, int64_t value);

/* ------------------------------------------------------------------------------------------------
 * Related notes (opt-in): NoteSimilarityCalculator.find_related_notes (utils/note_similarity.py:115-233) on the stored
 * rows of a normalising inner-product index — the N x N cosine_similarity matrix of :144 and the double loop of
 * _find_related_for_note (:169-233) with _calculate_entity_similarity (:235-259), without the matrix and without the
 * loop.  DESIGN.md §5m has the semantics, the error band and the strip passes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_related_params {
  double threshold;              /* similarity_threshold: a pair is kept when combined > threshold (strict, :210) */
  double entity_weight;          /* entity_similarity_weight w */
  double cluster_bonus;          /* cluster_similarity_bonus */
  int32_t min_shared;            /* min_shared_entities */
  int32_t exclude_same_cluster;  /* 0 / 1 */
  int32_t max_related;           /* max_related_notes M, 1 .. 64 */
  int32_t reserved;
} anr_related_params;
/* Replaces utils/note_similarity.py:142-144 and :174-221 for all rows at once.  For rows i != j:
 *   base     = the float64 dot product of the two stored float32 rows: the products exact, added per lane l = k mod 8 in
 *              ascending k, the eight sums joined as ((0+4)+(2+6)) + ((1+5)+(3+7)); no fused multiply-add.  The value depends
 *              on the two rows alone: equal stored rows give bit-equal values against any third row (:191);
 *   ent      = 0.5 if both entity rows are empty, 0.0 if one is, else min(inter / uni + (inter >= min_shared ? 0.1 : 0), 1.0)
 *              in float64 from the two integers (:235-259);
 *   cb       = cluster_bonus iff !exclude_same_cluster && c_i != c_j && base > threshold - 0.1, else 0 (:197-201);
 *   combined = base * (1 - w) + ent * w + cb, left to right in float64 (:204-208);
 *   skipped when exclude_same_cluster && c_i == c_j && c_i != -1 (:187); kept when combined > threshold (:210).
 * Row i receives its first M kept pairs by (combined descending, column ascending) — the reference's stable
 * sort(reverse = True) over ascending columns (:219-221).  Pairs are nominated by an MFMA walk of the f16 image with the
 * image's error band subtracted from the smallest base that can still pass, so no passing pair is lost; every value is
 * then taken from the float32 rows.  No floating-point atomics: the result does not depend on the order in which pairs
 * were found, nor on the pair capacity, and two calls are bit-equal.
 * cluster: int32 [ntotal] codes compared by equality, -1 = no cluster; NULL = all -1.  ent_indptr int64 [ntotal + 1] from 0,
 * ent_ids int32 STRICTLY ASCENDING and >= 0 inside a row (note_relations.encode_rows).
 * Outputs (host): nbr int32 [ntotal][M] (unused slots -1), n_nbr int32 [ntotal]; combined / base float64 and inter / uni
 * int32 [ntotal][M] (unused slots 0; each of the four may be NULL).
 * stats8 (may be NULL), int64 [8]: 0 pairs nominated by all walks (those of a strip that had to be cut again included),
 * 1 pairs scored, 2 pairs kept (i < j), 3 strips, 4 pair capacity, 5 nominated pairs the f16 image could not decide
 * (inside the band), 6 device scratch bytes of the call, 7 zero.
 * ANR_EINVAL: an L2 index, an inner-product index without normalisation, M outside [1, 64], a NaN parameter, an entity row
 * that descends or repeats an id, a negative id, ent_indptr not ascending from 0, ntotal >= 2^31 - 1.  ANR_ESTATE: a stored
 * value is outside the f16 range.  ntotal == 0: ANR_OK, nothing written. */
int anr_index_related_notes(anr_index *h, const anr_related_params *p, const int32_t *cluster, const int64_t *ent_indptr,
                            const int32_t *ent_ids, int32_t *nbr, int32_t *n_nbr, double *combined, double *base,
                            int32_t *inter, int32_t *uni, int64_t *stats8);
/* option 1 = ANR_RELATED_OPT_PAIR_CAP — the pairs one walk of anr_index_related_notes may nominate (process-wide; 0 = the
 * default: 64 pairs a row, within a quarter of the free device memory).  A walk that would nominate more is cut into strips of rows, each strip
 * walked, scored and merged into the per-row top M kept so far; the capacity is never below ntotal, the most one row can
 * nominate.  Tests force a small one to walk the strips on small inputs.  Results never depend on it.  Replaces nothing of
 * the reference: utils/note_similarity.py:144 holds the whole matrix. */
#define ANR_RELATED_OPT_PAIR_CAP 1
int anr_related_set_option(int32_t option, int64_t value);
/* Developer timing of anr_index_related_notes (tools/related_perf.py; process-wide, not for concurrent callers; the
 * reference has no counterpart, its loop is utils/note_similarity.py:182-216): enable != 0 makes later calls record HIP
 * events; ms3 (may be NULL) receives the last timed call's milliseconds summed over its strips: [0] the nominating walks,
 * [1] pair scoring, [2] sort and per-row selection. */
int anr_related_timing(int32_t enable, float *ms3);

/* ------------------------------------------------------------------------------------------------
 * TF-IDF cosine join and search (opt-in): the N x N cosine_similarity matrix and the i < j loop of
 * NoteValidator._find_semantic_duplicates (utils/note_validator.py:363-393) without the matrix and without the loop, and
 * the per-document sums of VectorRetriever._bm25_search (vector_store/retriever.py:966-1002).  A handle holds one sparse
 * float64 matrix on one device: rows are notes, items are term labels.  Every value is a sum of products, one rounded
 * multiply and one rounded add each, in ascending label order: with the labels of anorag_hip.note_dedup.relabel_terms that
 * is sklearn's own value, bit for bit.  DESIGN.md §5o and the top of csrc/tfidf.hip.  Calls on one handle are serialised.
 * ---------------------------------------------------------------------------------------------- */
typedef struct anr_tfidf anr_tfidf;
/* Row r holds terms[indptr[r] .. indptr[r+1]) with values[...] beside them, labels STRICTLY ASCENDING in [0, n_terms).
 * ANR_EINVAL, before any device work, for a row that descends or repeats a label, a label out of range, a value that is not
 * finite or is negative, a row whose sum of squares exceeds 1 + 2^-20 (pass rows of unit length; all-zero and empty rows
 * are legal), and the size limits of anr_setjoin_create. */
int anr_tfidf_create(int32_t device, int64_t n_rows, int64_t n_terms, const int64_t *indptr, const int32_t *terms,
                     const double *values, anr_tfidf **out);
int anr_tfidf_destroy(anr_tfidf *h);
/* Every pair i < j whose dot product s = (((0.0 + x_i0 * x_j0) + x_i1 * x_j1) + ...) over the shared labels ascending, in
 * float64 without fused multiply-add, is >= threshold.  threshold <= 0, NaN and > 2 are ANR_EINVAL: a pair that shares no
 * term is never looked at.  Pairs are nominated by an integer upper bound of 2^30 * s that cannot miss a passing pair and
 * decided by the exact value; two calls are bit-equal.  The result stays on the handle until the next call; *n_pairs (may be
 * NULL) = the pairs kept.  A nominated set that does not fit in the device's free memory is ANR_EHIP, never a truncation.
 * stats8 (may be NULL), int64 [8]: 0 rows that had candidates, 1 candidate insertions into the table, 2 pairs nominated,
 * 3 pairs kept, 4 rows_overflowed (more than one pass of the table), 5 table slots, 6 microseconds of the nominating stage
 * and 7 of the deciding stage (HIP events on the handle's stream). */
int anr_tfidf_self_join(anr_tfidf *h, double threshold, int64_t *n_pairs, int64_t *stats8);
/* the pairs sorted by (i, j), the order of the reference's loop (:382-386), with their values.  ANR_ESTATE before a join. */
int anr_tfidf_self_join_fetch(anr_tfidf *h, int32_t *I /*[n_pairs]*/, int32_t *J, double *sim);
/* cosine_similarity(q, M) of retriever.py:983 for nq queries: out_host float64 [nq][n_rows], per document
 * 0.0 + q_weights[0] * m + q_weights[1] * m + ... over the terms of query q in the order given, one addition at a time;
 * a document none of the terms occurs in stays 0.0.  nq == 0 and a query with no terms are legal.  ANR_EINVAL for a label
 * outside [0, n_terms), a weight that is not finite, q_indptr not ascending from 0, nq * n_rows above 2^37. */
int anr_tfidf_scores(anr_tfidf *h, int64_t nq, const int64_t *q_indptr, const int32_t *q_terms, const double *q_weights,
                     double *out_host);
/* option 1 = ANR_TFIDF_OPT_TABLE_SLOTS: as ANR_SETJOIN_OPT_TABLE_SLOTS (a power of two in [64, 4096], 0 = the default);
 * results never depend on it. */
#define ANR_TFIDF_OPT_TABLE_SLOTS 1
int anr_tfidf_set_option(anr_tfidf *h, int32_t option, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* ANORAG_H */
