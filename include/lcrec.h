/*
 * lcrec.h -- C-ABI of the MI355X (gfx950) implementation of LC-Rec's
 * item-indexing hot path.
 *
 * The reference (jiaozihao18/LC-Rec) is pure Python/PyTorch and has no FFI
 * layer; the seam this library sits under is the reference's nn.Module API
 * (SURVEY.md section 8b).  Each entry point below names the reference code it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is a HIP device
 *     pointer to a contiguous row-major buffer owned by the caller;
 *     pointers marked "host" are ordinary host arrays (shape descriptors);
 *   - the library allocates nothing that outlives a call: scratch space is a
 *     caller-provided workspace whose size is returned by *_workspace().  The one
 *     exception is explicit: an lcrec_context (create/destroy below) owns the helper
 *     streams, events and the pinned upload ring that the two calls taking a context
 *     may use; with a NULL context those calls keep every launch on `stream`;
 *   - all work is enqueued on `stream` (a hipStream_t, NULL = default stream), or on
 *     a context's helper streams forked from it and joined back into it before the
 *     call returns (on every exit path, errors included): a call is ordered after
 *     prior and before later work on `stream`; calls do not synchronise the device
 *     (the one documented host wait: lcrec_sinkhorn_assign with many groups and a
 *     NULL context);
 *   - no global mutable state apart from the diagnostic trace log; a context is used
 *     by one host thread at a time (one process per GPU needs no locking).  The library
 *     reads a handful of environment variables ONCE per process, on the first call that
 *     consults them (function-local statics): they select between kernels that compute
 *     the same bits and exist for A/B measurements, not for configuration --
 *       LCREC_GEMM_PP, LCREC_GEMM_PP3, LCREC_GEMM_FAST, LCREC_GEMM_S16, LCREC_GEMM_S16_TILES
 *                                  which tiling / kernel form lcrec_linear_forward (and the
 *                                  dX product of lcrec_linear_backward) takes
 *       LCREC_GEMM_SPLITK           cap on the K-runs of the weight gradient (changes S of
 *                                  lcrec_linear_backward_splits, hence its documented sum)
 *       LCREC_RQ_SPLIT              the batch-sized form of lcrec_rq_assign
 *       LCREC_SINKHORN_SCALING, LCREC_SINKHORN_PERSISTENT, LCREC_SK_RW, LCREC_SK_BLOCKS,
 *       LCREC_SK_LOCAL              which batch-sized Sinkhorn solver runs, and whether its
 *                                  exchange stays inside one XCD (assignments may differ only
 *                                  inside the 1e-9 margin stated at the call)
 *       LCREC_STRIP_COLS, LCREC_BN_V4, LCREC_BN_CACHED_MIN
 *                                  strip width / kernel form of the BatchNorm column reductions
 *                                  (the forms sum a column's rows in different orders: last-bit
 *                                  differences in the statistics, within the stated tolerances)
 *     A deployment sets none of them; being process-global they are outside the
 *     per-call / per-context contract above;
 *   - return 0 on success, a negative LCREC_E* code otherwise; the message for
 *     the calling thread's last error is lcrec_last_error(); nothing throws;
 *   - arithmetic contract: every contraction is one fp32 fused-multiply-add
 *     chain over k ascending starting at 0 (v_mfma_f32_32x32x2_f32 semantics);
 *     results are bit-identical to oracle/lcrec_oracle.c.  One documented
 *     exception: the weight gradient of lcrec_linear_backward is an ordered sum
 *     of a few such chains over runs of the batch (see there);
 *   - `ticket` arguments (ABI 3): a device pointer to ONE 4-byte word owned by the caller, or NULL.
 *     The word must be zero before its first use and every call that takes it leaves it zero.
 *     A call that sums per-workgroup partials finishes that sum in a second, one-workgroup launch;
 *     given a ticket, the workgroups count their arrivals in it and the last one to arrive adds
 *     the partials instead -- in the same order, so the result has the same bits -- and the second
 *     launch disappears (a training step makes ~80 launches and a fifth of them are such tails,
 *     4-5 us each).  Nothing waits on the word, so the dispatch order cannot deadlock a call.
 *     Calls that share a ticket must be ordered on one stream (or one captured graph branch).
 */
#ifndef LCREC_H
#define LCREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCREC_ABI_VERSION 3

#define LCREC_OK 0
#define LCREC_EINVAL (-1)      /* bad argument (shape, NULL pointer, unsupported size) */
#define LCREC_EUNSUPPORTED (-2) /* valid request this build has no kernel for */
#define LCREC_EWORKSPACE (-3)  /* workspace too small */
#define LCREC_EHIP (-4)        /* HIP runtime error (launch failed, no gfx950 device) */

#define LCREC_MAX_LEVELS 16
#define LCREC_MAX_LAYERS 16

/* LCREC_ABI_VERSION of the loaded library. */
int lcrec_version(void);

/* Message for the last error returned on the calling thread ("" if none). */
const char *lcrec_last_error(void);

/* Opaque per-device resources for the calls that can overlap independent launches (SURVEY.md section 8b:
 * "nothing persistent except an opaque handle with explicit create/destroy").  The reference has no
 * counterpart: its index/ stage issues every op on one stream (index/main.py:38, one device).
 * A context belongs to the HIP device that is current when it is created and holds
 *   - two helper streams with their fork/join events: ONE pool shared by the chunk pipelines of
 *     lcrec_encode_assign and the size-class launches of lcrec_sinkhorn_assign (so a process never owns
 *     more than two library streams per device, whatever mix of calls it makes);
 *   - a ring of pinned host buffers through which lcrec_sinkhorn_assign uploads its group table without
 *     waiting on the host;
 *   - settings: the number of chunk pipelines of lcrec_encode_assign (1 or 2; default 1).
 * Streams, events and pinned buffers are created on first use and released by lcrec_context_destroy,
 * which first waits for the helper streams to drain. */
typedef struct lcrec_context lcrec_context;
int lcrec_context_create(lcrec_context **out);
int lcrec_context_destroy(lcrec_context *ctx);
/* chunk pipelines of lcrec_encode_assign: 1 (default) = every launch on the caller's stream; 2 = odd chunks on a helper
 * stream: +1.5-1.9 % on C3 when the two streams' persistent GEMM launches share the CUs evenly, but the hardware dispatcher
 * sometimes starves one of them (measured: a 61 ms pass taking 101 ms, round 1: 185 ms), so it is opt-in. */
int lcrec_context_set_pipelines(lcrec_context *ctx, int pipelines);

/* One MLP layer: y = [relu]( [bn]( x @ W^T + b ) ).
 * Replaces one Dropout(p=0)/Linear/[BatchNorm1d eval]/[ReLU] group of
 * MLPLayers.forward, index/models/layers.py:18-30,42 (nn.Linear at :23,
 * BatchNorm1d at :26, activation at :28-30).
 *   x [n][in_dim], W [out_dim][in_dim] (nn.Linear.weight layout), b [out_dim] or NULL,
 *   bn_scale/bn_shift [out_dim] or both NULL: eval-mode BatchNorm folded by the
 *   caller to y = t*scale + shift (scale = gamma/sqrt(var+eps), shift = beta - mean*scale),
 *   y [n][out_dim].  All device pointers. */
int lcrec_linear_forward(const float *x, int64_t n, int in_dim, const float *W, const float *b,
                         const float *bn_scale, const float *bn_shift, int relu, int out_dim,
                         float *y, void *stream);

/* One Linear of a TRAINING step with the BatchNorms on either side of it folded in (index/models/layers.py:23-30 in train();
 * the reference runs Linear, BatchNorm1d and ReLU as three modules with a full activation tensor between each pair):
 *   u = x * in_scale + in_shift, clamped at 0 from below when in_relu != 0   (in_scale / in_shift [in_dim], both NULL: u = x)
 *         -- the PREVIOUS layer's BatchNorm + ReLU, applied while the operand tile is staged: that layer's activation
 *            is never written, its pre-BatchNorm output is all that exists;
 *   t_out [n][out_dim] = u @ W^T + b   (the same fp32 fma chains as lcrec_linear_forward, bit for bit, on u);
 *   want_stats != 0: the batch statistics of t_out over its n rows -- THIS layer's BatchNorm (layers.py:26) -- taken in the
 *         product's epilogue: mean_out, rstd_out = 1/sqrt(biased var + eps), scale_out = gamma * rstd, shift_out = beta -
 *         mean * scale_out (what the next lcrec_linear_bn_forward takes as in_scale / in_shift), and running_mean /
 *         running_var (may be NULL) updated with `momentum` as nn.BatchNorm1d does (unbiased variance).  gamma / beta may
 *         be NULL (1 / 0).  Every tile publishes per-column partial sums; the last tile of a column strip to arrive merges
 *         them in tile order (deterministic; see "ticket arguments"): tickets = ceil(out_dim / 64) zeroed words, left zero.
 *   workspace: lcrec_linear_bn_forward_workspace(n, out_dim) bytes (want_stats only).
 * Batch-sized launches only (n <= a few thousand rows: the tile rule of a training step), in_dim % 32 == 0, out_dim % 4 == 0,
 * out_dim <= 4096; anything else returns LCREC_EUNSUPPORTED and the caller uses lcrec_linear_forward + lcrec_bn_relu_forward.
 * Statistics agree with torch's to ~1e-7 relative (another summation order); pinned by fixtures F4 and F11 through the engine. */
size_t lcrec_linear_bn_forward_workspace(int64_t n, int out_dim);
int lcrec_linear_bn_forward(const float *x, int64_t n, int in_dim, const float *in_scale, const float *in_shift, int in_relu,
                            const float *W, const float *b, int out_dim, float *t_out, int want_stats, const float *gamma,
                            const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                            float *mean_out, float *rstd_out, float *scale_out, float *shift_out, void *workspace,
                            size_t workspace_bytes, unsigned int *tickets, void *stream);

/* The two backward products of one Linear layer, as autograd derives them for nn.Linear in
 * MLPLayers (index/models/layers.py:23; driven by loss.backward() at index/trainer.py:117,
 * SURVEY.md row a9):
 *   gx [n][in_dim]       = gy [n][out_dim] * W [out_dim][in_dim]
 *   gw [out_dim][in_dim] = gy^T * x [n][in_dim]
 * gy is the gradient w.r.t. the layer's pre-activation output (the caller has already applied the
 * ReLU mask); the bias gradient is the caller's column sum of gy.  Every operand is read in the
 * layout it is stored in -- no transposed copies -- and every output element is one fp32 fma chain
 * over the contracted index ascending (out_dim for gx), like the forward kernel.  For gw the
 * contracted index is the batch: it is cut into S = lcrec_linear_backward_splits(n, in_dim, out_dim)
 * runs of 32*ceil(ceil(n/32)/S) consecutive items (S = 1 for the wide layers, up to 16 for the narrow
 * ones, so that a small [out_dim][in_dim] output still fills the chip); each run is one fma chain
 * from 0 and the runs are added in order, ((p0 + p1) + p2) + ...  S depends only on the three sizes.
 * gx_out / gw_out may be NULL to skip a product.  out_dim % 32 == 0 is required for gx, in_dim and
 * out_dim % 4 == 0 for both; sized for training batches (n * max(in_dim, out_dim) < 2^29).
 * workspace: device scratch of lcrec_linear_backward_workspace() bytes (S partial products; 0 if S = 1). */
int lcrec_linear_backward_splits(int64_t n, int in_dim, int out_dim);
size_t lcrec_linear_backward_workspace(int64_t n, int in_dim, int out_dim);
int lcrec_linear_backward(const float *gy, const float *x, const float *W, int64_t n, int in_dim, int out_dim,
                          float *gx_out, float *gw_out, void *workspace, size_t workspace_bytes, void *stream);

/* The weight gradients of SEVERAL Linear layers in one launch: gw_p = gy_p^T * x_p for p < count (count <= 16), each
 * exactly what lcrec_linear_backward computes for that layer -- the same S = lcrec_linear_backward_splits runs, added in
 * order -- so the results are bit-identical to per-layer calls.  A training step's narrow layers are a handful of tiles
 * each; launched together their workgroups fill the chip (index/trainer.py:117: autograd produces these one at a time).
 * A problem's `splits` field (> 0) sets its S itself -- the same definition of the runs and of their sum, another S.  A
 * launch of a whole step's problems has thousands of tiles, and cutting the narrow layers' batches there only adds partial
 * products to write, read and add (the training engine passes 1: one fma chain over the batch per element).
 * `problems` is a HOST array; all pointers inside are device pointers.  Widths must be multiples of 4. */
typedef struct {
    const float *gy;   /* [n][out_dim] gradient w.r.t. the layer's pre-activation output */
    const float *x;    /* [n][in_dim]  the layer's input */
    float *gw;         /* [out_dim][in_dim] */
    int64_t n;
    int in_dim, out_dim;
    /* ABI 3: both NULL, or [in_dim] device vectors: the layer's input is then u = x * x_scale + x_shift, clamped at 0 from
     * below when x_relu != 0 -- x being the PRE-BatchNorm output of the previous layer as lcrec_linear_bn_forward leaves it
     * and (x_scale, x_shift) that BatchNorm's folded affine; u is formed on the operand's way into LDS. */
    const float *x_scale, *x_shift;
    int x_relu;
    int splits;        /* ABI 3: 0 = S of lcrec_linear_backward_splits(n, in_dim, out_dim); > 0 = this S (at most ceil(n/32)) */
} lcrec_dw_problem;
size_t lcrec_linear_backward_weights_workspace(const lcrec_dw_problem *problems, int count);
int lcrec_linear_backward_weights(const lcrec_dw_problem *problems, int count, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* L-level residual quantisation with hard (argmin) assignment.
 * Replaces ResidualVectorQuantizer.forward, index/models/rq.py:39-55, over
 * VectorQuantizer.forward with use_sk=False, index/models/vq.py:63-99
 * (distance :71-73, argmin :75, gather :87, losses :90-92, STE :95).
 *   z          device [n][e]         latents
 *   codebooks  device, level l is [K[l]][e] at float offset sum_{m<l} K[m]*e
 *                                    (= torch.cat of rq.get_codebook() rows, rq.py:32-37)
 *   K          host   [L]            codes per level (any positive count; a level must fit
 *                                    in LDS: roundup32(K)*(e+5)*4 bytes <= ~156 KB)
 *   idx_out    device int64, item i's level-l code at idx_out[i*idx_stride + l] (rq.py:54);
 *   idx_stride elements between rows, >= L; 0 = L (a dense [n][L] matrix).  A run of levels can so be
 *                                    written straight into the columns of a wider index matrix
 *   xq_out     device [n][e] or NULL sum over levels of the straight-through x_res (rq.py:48);
 *                                    if xq_accumulate != 0 its current contents are the initial
 *                                    value of the sum (chaining a run of levels after another)
 *   sse_out    device [L] double or NULL  per-level sum of (c - r)^2; the level loss of
 *                                    vq.py:90-92 is (1+beta)*sse/(n*e)
 *   resid_out  device [L+1][n][e] or NULL  entry l = residual fed into level l (input of
 *                                    lcrec_code_stats), entry L = residual after the last level
 *   margin_out device [n][L] float or NULL  near-tie audit: per item and level, the second smallest
 *                                    distance minus the smallest, both as computed above (0 on an exact
 *                                    tie, +inf when K[l] == 1)
 *   neartie_out device [n] uint32 or NULL   bit l set when margin_l <= tie_tau * (xx_l + cc_l[idx_l]),
 *                                    the magnitude at which the winning distance of level l was rounded
 *   tie_tau    threshold for neartie_out (>= 0; ignored when neartie_out is NULL)
 *   workspace  device scratch of lcrec_rq_assign_workspace() bytes
 *   ticket     NULL, or see "ticket arguments" above (finishes sse_out inside the launch)
 * e must be 16, 32 or 64.
 * Why the audit outputs exist: the reference decides vq.py:75 on fp32 distances whose summation order (MKL,
 * vectorised reductions) is unspecified and batch-size dependent (hard part 1), so an item
 * whose two best codes are closer than that noise can get a different code from the reference's CPU run than from
 * this library's canonical order -- and, its residual then differing, different codes on the levels after it.
 * Items whose neartie_out is 0 at the tau recorded in tests/golden/f9_neartie_*.npz carry the reference's tuple;
 * DESIGN.md section 2 states the measured rates. */
size_t lcrec_rq_assign_workspace(int64_t n, int e, const int *K, int L);
int lcrec_rq_assign(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L,
                    int64_t *idx_out, int64_t idx_stride, float *xq_out, int xq_accumulate, double *sse_out,
                    float *resid_out, float *margin_out, uint32_t *neartie_out, float tie_tau,
                    void *workspace, size_t workspace_bytes, unsigned int *ticket, void *stream);

/* Encoder MLP + residual quantisation: item embeddings -> index tuples.
 * Replaces RQVAE.get_indices(xs, use_sk=False), index/models/rqvae.py:68-72
 * (encoder = MLPLayers, layers.py:42; rq = rq.py:39-55).  This is the path
 * BASELINE.json's metric measures.
 *   x          device [n][dims[0]]
 *   dims       host   [n_layers+1]   in_dim, hidden sizes..., e_dim (rqvae.py:46)
 *   W, b, bn_scale, bn_shift  host arrays of n_layers device pointers (bn_* arrays
 *              may be NULL, or hold NULL entries for layers without BatchNorm);
 *              ReLU follows every layer but the last (layers.py:27-30)
 *   latent_out device [n][e] or NULL  encoder output
 *   others     as lcrec_rq_assign (margin_out / neartie_out / tie_tau: the near-tie audit of the quantiser)
 *   ctx        NULL, or a context of the current device
 * Items are processed in chunks of lcrec_encode_assign_chunk_rows() = 524 288.  With a context whose pipelines setting is 2 (opt-in), odd chunks run on
 * the context's first helper stream, forked from `stream` by an event at entry and joined back into it before
 * the quantiser pass (and on every error exit), so everything is ordered after prior work on `stream` and
 * before later work on it, without any host synchronisation; with ctx == NULL or pipelines == 1 every launch
 * is on `stream`.  The walk and the layout of the workspace are one host function's decision, which
 * lcrec_debug_encode_assign_plan (below, debug entries) reports.
 * lcrec_encode_assign_workspace returns 0 for arguments lcrec_encode_assign refuses. */
size_t lcrec_encode_assign_workspace(int64_t n, const int *dims, int n_layers, const int *K, int L);
/* rows per chunk of the walk described above (a build constant; results do not depend on it) */
int64_t lcrec_encode_assign_chunk_rows(void);
int lcrec_encode_assign(const float *x, int64_t n, const int *dims, int n_layers,
                        const float *const *W, const float *const *b,
                        const float *const *bn_scale, const float *const *bn_shift,
                        const float *codebooks, const int *K, int L, int64_t *idx_out,
                        float *latent_out, float *xq_out, double *sse_out,
                        float *margin_out, uint32_t *neartie_out, float tie_tau,
                        void *workspace, size_t workspace_bytes, lcrec_context *ctx, void *stream);

/* Sinkhorn ("uniform semantic") assignment of one level, for one or many independent
 * groups of rows.  Replaces the use_sk branch of VectorQuantizer.forward,
 * index/models/vq.py:76-83: distances (:71-73, same fp32 fma chains as lcrec_rq_assign),
 * centring on the group's global max/min (:51-61), fp64 sinkhorn_algorithm
 * (index/models/layers.py:85-108: Q=exp(-d/eps), /total, iters x {/rowsum, /B, /colsum, /K},
 * *B, every division a true fp64 division in that order) and argmax (:83, first maximum).
 * Training calls it with one group (the batch, index/trainer.py:114); index generation
 * with one group per set of colliding items (index/generate_indices.py:113-119), which the
 * reference runs one forward at a time and this runs as one batched launch.
 *   resid          device [n][e]   residual entering the level
 *   codebook       device [K][e]
 *   group_offsets  HOST  [n_groups+1] ascending row offsets; group g = rows [off[g], off[g+1])
 *   idx_out        device int64, element i written at idx_out[i*idx_stride]
 *   ctx            NULL, or a context of the current device
 * e must be 16, 32 or 64; K <= 1024 for groups too large for LDS (rows*K > 16384).
 * With several groups the call buckets them by size, one launch per bucket.  With a context the buckets go to
 * `stream` and to the context's two helper streams, forked from `stream` by an event and joined back into it
 * before the call returns (error exits included), and the group table reaches the device through the context's
 * pinned ring: no host wait.  With ctx == NULL every launch is on `stream` and the call waits once on the host
 * for the upload of the group table (many-group calls only; a single training batch never synchronises).
 * A lone group of more than 16384/K rows is solved by one multi-workgroup launch whose workgroups must all be
 * resident: it is chosen only when the occupancy the runtime reports for its LDS size times the CU count covers
 * the grid (<= 128 workgroups), otherwise the multi-launch solver runs; every spin in it is bounded (~0.1 s in
 * total) and a timeout -- other work holding the CUs -- fills idx_out with -1 instead of hanging.
 * ticket (NULL, or see "ticket arguments"): the batch-sized solver's control words and exchange slots are then set up by the
 * distance launch itself (its last workgroup reduces the global max/min of vq.py:52-53 from the workgroups' partials) instead
 * of by a launch of their own in front of it. */
size_t lcrec_sinkhorn_assign_workspace(int64_t n, int K, const int64_t *group_offsets, int n_groups);
int lcrec_sinkhorn_assign(const float *resid, int64_t n, int e, const float *codebook, int K,
                          const int64_t *group_offsets, int n_groups, double epsilon, int iters,
                          int64_t *idx_out, int64_t idx_stride, void *workspace, size_t workspace_bytes,
                          lcrec_context *ctx, unsigned int *ticket, void *stream);

/* Apply a given assignment to one level: gather, squared error, straight-through estimator and
 * residual update (index/models/vq.py:87-95, index/models/rq.py:47-48) -- what follows the
 * argmin/argmax inside VectorQuantizer.forward, for levels whose indices came from
 * lcrec_sinkhorn_assign.
 *   xq        device [n][e] or NULL: x_q sum, += x_res (starts from 0 unless xq_accumulate)
 *   resid_out device [n][e] or NULL: residual after the level (may alias resid_in)
 *   sse_out   device double[1] or NULL; workspace must then hold 8 KB
 *   ticket    NULL, or see "ticket arguments" (finishes sse_out inside the launch)
 * A code outside [0, K): below 0 counts as 0, K and above as K - 1, decided on the int64 value (a batch-sized
 * lcrec_sinkhorn_assign that gives up fills its column with -1).  lcrec_code_stats and lcrec_code_stats_levels take the
 * same rule, so the statistics are those of the squared error this call computed. */
int lcrec_rq_apply_level(const float *resid_in, int64_t n, int e, const float *codebook, int K,
                         const int64_t *idx, int64_t idx_stride, float *xq, int xq_accumulate,
                         float *resid_out, double *sse_out, void *workspace, size_t workspace_bytes,
                         unsigned int *ticket, void *stream);

/* Per-code count and sum of the residuals assigned to it:
 *   count[k] = #{i : code(i) == k},  sum[k][:] = sum_i resid[i][:]  (item order, fp32),
 *   code(i) = idx[i*idx_stride] brought into [0, K-1] by the rule of lcrec_rq_apply_level: below 0 counts as 0, K and
 *   above as K - 1, decided on the int64 value -- for every n, whichever kernel the size selects.
 * Replaces the scatter_add_/index_add_ block of index_improve/models/vq.py:151-167 and is the
 * segmented reduce behind the codebook gradient autograd derives from vq.py:90-92
 * (dL/dC[k] = w * (count[k]*C[k] - sum[k])).  Bit-identical to the CPU order. */
int lcrec_code_stats(const int64_t *idx, int64_t idx_stride, const float *resid, int64_t n, int e, int K,
                     float *count, float *sum, void *stream);

/* lcrec_code_stats for ALL levels of a quantiser in one launch, optionally fused with lcrec_codebook_grad:
 *   idx      device [n][L] int64 (ResidualVectorQuantizer's index matrix, rq.py:54)
 *   resid    HOST array of L device pointers, resid[l] [n][e] = the residual that entered level l
 *   K        HOST [L];  count / sum: HOST arrays of L device pointers ([K[l]], [K[l]][e])
 *   codebooks / grad_out: both NULL, or HOST arrays of L device pointers: grad_out[l] =
 *            (scale * (count*C_l - sum)) * weight, see lcrec_codebook_grad
 * Same bits as the per-level calls, codes outside [0, K[l]) included (the rule of lcrec_rq_apply_level). */
int lcrec_code_stats_levels(const int64_t *idx, const float *const *resid, int64_t n, int e, const int *K, int L,
                            float *const *count, float *const *sum, const float *const *codebooks, float *const *grad_out,
                            float scale, float weight, void *stream);

/* EMA codebook update, index_improve/models/vq.py:155-184, in place:
 *   ema_count = ema_count*decay + alpha*count;  ema_sum = ema_sum*decay + alpha*sum;
 *   where ema_count > eps:  codebook = codebook*keep + (ema_sum/(ema_count+eps))*alpha.
 * decay, alpha = 1-decay and keep = 1-(1-decay) are the reference's python doubles rounded to fp32
 * by the caller.  skip_flag: NULL, or a device byte; when it is non-zero the call changes nothing (the sticky
 * "loss was NaN" flag of lcrec_step_losses: the reference raises before the offending step updates anything,
 * index/trainer.py:116, so a caller that learns of the NaN later still finds the last good state). */
int lcrec_ema_update(float *ema_count, float *ema_sum, float *codebook, const float *count,
                     const float *sum, int K, int e, float decay, float alpha, float keep, float eps,
                     const unsigned char *skip_flag, void *stream);

/* ---- the element-wise / column-reduction half of a training step -------------------
 * Device pointers throughout; batch-sized inputs (n <= 2^20 rows); deterministic (no atomics): a column is summed by
 * 8 row groups (rows r = g, g+8, ... in order) whose partials are added in group order.  Floating-point results are
 * within 1e-5 of the torch ops they replace (the reference's own order is unspecified); pinned by the reference's
 * F4 three-step trajectory. */

/* Training-mode BatchNorm1d (+ ReLU) on the output t [n][features] of a Linear: index/models/layers.py:25-30
 * (nn.BatchNorm1d at :26 in train(), activation at :28-30).  Batch mean and biased variance (two passes), y =
 * [relu]((t - mean) * rstd * gamma + beta), rstd = 1/sqrt(var + eps); running_mean / running_var (may be NULL) are
 * updated in place with `momentum`, running_var from the unbiased variance; mean_out / rstd_out [features] are what
 * the backward needs.  n >= 2. */
int lcrec_bn_relu_forward(const float *t, int64_t n, int features, const float *gamma, const float *beta, float eps,
                          float momentum, float *running_mean, float *running_var, float *y, float *mean_out,
                          float *rstd_out, int relu, void *stream);

/* Backward of the above for gy = dL/dy (what autograd derives for layers.py:25-30 under loss.backward(),
 * index/trainer.py:117):  g = gy * [y > 0];  dbeta = sum g;  dgamma = sum g*xhat;
 * dt = gamma*rstd*(g - dbeta/n - xhat*dgamma/n);  dbias = sum dt -- the gradient of the Linear bias feeding the
 * BatchNorm (zero up to rounding, as in the reference).  dgamma/dbeta/dbias may be NULL; dt may alias gy.
 * y may be NULL when relu != 0 and fold_scale / fold_shift [features] are given: the mask is then [t * fold_scale +
 * fold_shift > 0] (one fma), the expression the consumer of lcrec_linear_bn_forward's output evaluated.  With y NULL,
 * fold_scale NULL and fold_shift = the layer's beta [features], the mask is [(t - mean) * rstd * gamma + beta > 0]
 * evaluated exactly as lcrec_bn_relu_forward evaluates y: the same bits as passing that y, one array less to read. */
int lcrec_bn_relu_backward(const float *gy, const float *t, const float *y, int64_t n, int features, const float *gamma,
                           const float *mean, const float *rstd, int relu, float *dt_out, float *dgamma_out,
                           float *dbeta_out, float *dbias_out, const float *fold_scale, const float *fold_shift, void *stream);

/* The same two operations split where an item-sharded (data-parallel) run exchanges statistics, so that the batch is the
 * union of all ranks' rows (torch.nn.SyncBatchNorm semantics; the reference's index/ stage is single-process, SURVEY.md
 * section 8e item 4):
 *   lcrec_bn_stats            local mean and M2 = sum (t - mean)^2 of this rank's n rows      -> exchanged by the caller
 *   lcrec_bn_merge_stats      rows[world][2*features+1] = every rank's (n_r, mean_r[], M2_r[]) -> mean, rstd of the union of
 *                             the rows (Chan et al., merged in rank order: the same bits on every rank) and the running
 *                             statistics as nn.BatchNorm1d keeps them (running_* may be NULL)
 *   lcrec_bn_relu_apply       y = [relu]((t - mean) * rstd * gamma + beta) with the merged statistics
 *   lcrec_bn_backward_reduce  local sum g and sum g*xhat (g = gy * [y > 0])                    -> all-reduced by the caller;
 *                             dbeta_out / dgamma_out (may be NULL) receive a copy: this rank's share of the parameter gradients
 *   lcrec_bn_backward_apply   dt = gamma*rstd*(g - sum_g/n_total - xhat*sum_gx/n_total), dbias = local column sums of dt */
int lcrec_bn_stats(const float *t, int64_t n, int features, float *mean_out, float *m2_out, void *stream);
int lcrec_bn_merge_stats(const float *rows, int world, int features, float eps, float momentum, float *mean_out, float *rstd_out,
                         float *running_mean, float *running_var, void *stream);
int lcrec_bn_relu_apply(const float *t, int64_t n, int features, const float *gamma, const float *beta, const float *mean,
                        const float *rstd, int relu, float *y, void *stream);
int lcrec_bn_backward_reduce(const float *gy, const float *t, const float *y, int64_t n, int features, const float *mean,
                             const float *rstd, int relu, float *sum_g_out, float *sum_gx_out, float *dbeta_out,
                             float *dgamma_out, void *stream);
int lcrec_bn_backward_apply(const float *gy, const float *t, const float *y, int64_t n, int features, const float *gamma,
                            const float *mean, const float *rstd, int relu, const float *sum_g, const float *sum_gx,
                            float n_total, float *dt_out, float *dbias_out, void *stream);

/* ReLU mask and bias gradient of a Linear without BatchNorm (layers.py:23,28-30): g = gy * [y > 0] (relu != 0;
 * g_out may alias gy or be NULL), dbias = column sums of g. */
int lcrec_relu_bias_backward(const float *gy, const float *y, int64_t n, int features, int relu, float *g_out,
                             float *dbias_out, void *stream);

/* Scratch (bytes) of the two whole-tensor reductions below. */
size_t lcrec_train_reduce_workspace(void);

/* Reconstruction loss and its gradient, index/models/rqvae.py:74-85: l1 == 0: loss = mean (out-x)^2,
 * grad = 2 (out-x)/count; l1 != 0: loss = mean |out-x|, grad = sign(out-x)/count.  count = n * in_dim elements;
 * loss_out is a device float (fp64 accumulation); grad_out [count] or NULL.
 * count_total (0 = count): the element count of the GLOBAL batch when these `count` elements are one rank's shard of
 * it (item-sharded data parallel): both divisions use count_total, so loss_out is this rank's share of the global
 * mean and the ranks' gradients sum to the global-batch gradient. */
int lcrec_recon_loss_grad(const float *out, const float *x, int64_t count, int64_t count_total, int l1, float *grad_out,
                          float *loss_out, void *workspace, size_t workspace_bytes, unsigned int *ticket, void *stream);

/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (index/trainer.py:118) on a flat gradient buffer:
 * norm_out[0] = ||grads||_2 (fp64 accumulation), norm_out[1] = min(1, max_norm / (norm + 1e-6)), the coefficient
 * lcrec_adamw_step applies. */
int lcrec_grad_norm_clip(const float *grads, int64_t count, float max_norm, float *norm_out, void *workspace,
                         size_t workspace_bytes, unsigned int *ticket, void *stream);

/* Codebook gradient from the per-code statistics of lcrec_code_stats -- what autograd derives from the two MSE terms
 * of index/models/vq.py:90-92: grad[k][:] = (scale * (count[k]*C[k][:] - sum[k][:])) * weight, with
 * scale = 2/(L*n*e) and weight = d loss / d rq_loss (quant_loss_weight, index/models/rqvae.py:83).  [K][e] each. */
int lcrec_codebook_grad(const float *count, const float *sum, const float *codebook, int K, int e, float scale,
                        float weight, float *grad_out, void *stream);

/* The scalar tail of a training step in one launch: level losses mse_l + beta*mse_l with mse_l = sse[l]/(n*e)
 * (index/models/vq.py:90-92), their mean (rq.py:53), loss = recon + quant_loss_weight * rq_loss (rqvae.py:83);
 * losses_out[3] = {loss, recon, rq_loss}; sums_inout[2] += {loss, recon} (trainer.py:122-123; may be NULL);
 * *nan_flag = 1 if the loss is NaN (trainer.py:116's check as a sticky device flag; may be NULL).  sse as written by
 * lcrec_rq_assign / lcrec_rq_apply_level (device double[L]); recon a device float (lcrec_recon_loss_grad).
 * poison_probe / poison_flag (both NULL, or both given): *poison_flag = 1 when *poison_probe < 0 -- the first assignment of a
 * batch-sized lcrec_sinkhorn_assign, which fills its output with -1 when its solver gives up; also sticky. */
int lcrec_step_losses(const double *sse, int L, int64_t n, int e, float beta, float quant_loss_weight, const float *recon,
                      float *losses_out, double *sums_inout, unsigned char *nan_flag, const int64_t *poison_probe,
                      unsigned char *poison_flag, void *stream);

/* Gradient reaching the encoder output z through the quantiser (autograd of vq.py:87-95 / rq.py:45-48):
 * out = (coef * (z - C0[idx0])) * weight + g_xq, coef = beta * 2/(L*n*e), weight = d loss / d rq_loss; idx0 = the
 * level-0 index column (element i at idx[i*idx_stride]); all [n][e]. */
int lcrec_quantizer_input_grad(const float *z, const float *codebook0, const int64_t *idx, int64_t idx_stride, int64_t n,
                               int e, float coef, float weight, const float *g_xq, float *out, void *stream);
/* The same, and dbias_out[e] = the column sums of `out`: the gradient of the bias of the encoder's last Linear, which has no
 * BatchNorm and no activation behind it (index/models/layers.py:19-30 skips both on the last layer), so what reaches z reaches
 * its pre-activation unchanged -- one launch for what lcrec_quantizer_input_grad + lcrec_relu_bias_backward(relu = 0) do in two.
 * dbias_out NULL: lcrec_quantizer_input_grad. */
int lcrec_quantizer_input_grad_bias(const float *z, const float *codebook0, const int64_t *idx, int64_t idx_stride, int64_t n,
                                    int e, float coef, float weight, const float *g_xq, float *out, float *dbias_out, void *stream);

/* One optimiser step on flat fp32 buffers: torch.optim.AdamW (decoupled != 0) or Adam (index/trainer.py:49-81,119),
 * preceded by the clipping of index/trainer.py:118 (grads *= clip[1], stored back; clip may be NULL) and with the
 * learning rate of index/trainer.py:83-92,120 evaluated on the device from the step counter:
 *   schedule -1: lr = base_lr;  0: constant after a linear warm-up;  1: linear warm-up, then linear decay to 0 at
 *   total_steps (transformers' get_{constant,linear}_schedule_with_warmup multipliers, in double).
 * *step (device int64) = optimiser steps taken so far; the call uses lr(*step) and bias corrections for step *step+1,
 * then increments it -- so a captured hipGraph of a training step replays without any host-side scalar.
 * lr_out: device float receiving the learning rate used, or NULL.
 * ticket: NULL, or see "ticket arguments": the increment is then made by the last workgroup of the update launch.
 * skip_flag: NULL, or a device byte; non-zero = update nothing and leave *step (see lcrec_ema_update).
 * base_lr and weight_decay must be >= 0, as for the other learners below (all four share one launcher; torch refuses
 * such an optimiser at construction).
 *
 * The arithmetic, per element (p param, m exp_avg, v exp_avg_sq): every op one fp32 rounding and, but for the lerp, none
 * fused; IEEE sqrt and division.  Each constant is computed in double from the double hyper-parameters and rounded to
 * float once; t = *step + 1, lr = lr(*step):
 *   g = grads * clip[1]                        stored back to grads when clip is given and clip[1] != 1
 *   weight_decay != 0, decoupled (AdamW):      p = p - (float)(lr * weight_decay) * p
 *   weight_decay != 0, not decoupled (Adam):   g = g + p * (float)weight_decay      (grads keeps the clipped value alone)
 *   m = m.lerp(g, w), w = (float)(1 - beta1)   torch's lerp: |w| < 0.5: fma(w, g - m, m), else fma(w - 1, g - m, g), w - 1 in float
 *   v = (float)beta2 * v + ((float)(1 - beta2) * g) * g
 *   denom = sqrt(v) / (float)sqrt(bc2) + (float)eps,        bc2 = 1 - pow(beta2, t)
 *   p = p - ((float)(lr / bc1) * m) / denom,                bc1 = 1 - pow(beta1, t)
 * exp_avg then has the bits of torch's single-tensor Adam (but under L2, which torch adds fused); torch decays AdamW's
 * parameters by p.mul_(1 - lr * weight_decay), so those differ from it in the last bit on about a third of the elements
 * (the learners). */
int lcrec_adamw_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t count, const float *clip,
                     int64_t *step, double base_lr, double beta1, double beta2, double eps, double weight_decay,
                     int decoupled, int schedule, int64_t warmup_steps, int64_t total_steps, float *lr_out,
                     unsigned int *ticket, const unsigned char *skip_flag, void *stream);

/* The reference's other learners (index/trainer.py:49-81,118-120) on flat fp32 buffers: the same kernel with another
 * rule, so around the rule everything is as for lcrec_adamw_step: grads *= clip[1] first (stored back when
 * clip[1] != 1; clip may be NULL), the learning rate lr(*step) from `schedule` / warmup_steps / total_steps, lr_out, the increment of *step (by the last
 * workgroup with a ticket, else by a second launch), and skip_flag (non-zero: update nothing, leave *step).  Per element,
 * g = grads * clip[1], then g += weight_decay * param when weight_decay != 0; the rules are torch 2.10's
 * _single_tensor_{sgd,adagrad,rmsprop}, with each op rounded as torch's CPU kernel rounds it (add with alpha and addcmul
 * fused, addcdiv as x + (value * y) / z, IEEE sqrt and division).  State is fp32, hyper-parameters are double.
 * The ops, a and w being double constants rounded to float once (so -lr is (float)(-lr), 1 - alpha is (float)(1 - alpha)):
 *   x.add(y, alpha=a)         fma(a, y, x)               x.mul(a), x + y, sqrt(x), x / y   one rounding each
 *   x.addcmul(y, z, value=a)  fma(a * y, z, x)           x.addcdiv(y, z, value=a)          x + (a * y) / z
 *   x.lerp(y, w)              |w| < 0.5: fma(w, y - x, x), else fma(w - 1, y - x, y), w - 1 in float
 * and the rules in them (g after the clipping and the weight decay g = g.add(param, alpha=weight_decay); grads keeps
 * the clipped value alone):
 *   SGD       buf = first ? g : buf.mul(momentum).add(g, alpha=1 - dampening);  g = nesterov ? g.add(buf, alpha=momentum) : buf;
 *             param = param.add(g, alpha=-lr)
 *   Adagrad   sum = sum.addcmul(g, g, value=1);  std = sqrt(sum) + eps;  param = param.addcdiv(g, std, value=-clr)
 *   RMSprop   sq = sq.mul(alpha).addcmul(g, g, value=1 - alpha);  centered: ga = ga.lerp(g, 1 - alpha),
 *             avg = sqrt(sq.addcmul(ga, ga, value=-1)) + eps, else avg = sqrt(sq) + eps;
 *             momentum > 0: buf = buf.mul(momentum).addcdiv(g, avg, value=1), param = param.add(buf, alpha=-lr),
 *             else param = param.addcdiv(g, avg, value=-lr)
 *
 * torch.optim.SGD: with momentum != 0, momentum_buffer[count] and momentum_ready (device byte) are required, otherwise
 * both are NULL.  momentum_ready == 0: buf = g (torch's first step) and the byte is set to 1 with the step increment;
 * else buf = momentum * buf + (1 - dampening) * g.  g = nesterov ? g + momentum * buf : buf.  param -= lr * g.
 * nesterov needs momentum > 0 and dampening == 0. */
int lcrec_sgd_step(float *params, float *grads, float *momentum_buffer, unsigned char *momentum_ready, int64_t count,
                   const float *clip, int64_t *step, double base_lr, double momentum, double dampening, int nesterov,
                   double weight_decay, int schedule, int64_t warmup_steps, int64_t total_steps, float *lr_out,
                   unsigned int *ticket, const unsigned char *skip_flag, void *stream);

/* torch.optim.Adagrad: clr = lr / (1 + *step * lr_decay) (torch's step counts this step), state_sum += g * g,
 * param += -clr * g / (sqrt(state_sum) + eps).  state_sum starts at initial_accumulator_value (the caller's fill). */
int lcrec_adagrad_step(float *params, float *grads, float *state_sum, int64_t count, const float *clip, int64_t *step,
                       double base_lr, double lr_decay, double eps, double weight_decay, int schedule, int64_t warmup_steps,
                       int64_t total_steps, float *lr_out, unsigned int *ticket, const unsigned char *skip_flag, void *stream);

/* torch.optim.RMSprop: square_avg = alpha * square_avg + (1 - alpha) * g * g; centered (grad_avg[count] given, else
 * NULL): grad_avg = lerp(grad_avg, g, 1 - alpha), avg = sqrt(square_avg - grad_avg^2) + eps; else avg = sqrt(square_avg)
 * + eps.  momentum > 0 (momentum_buffer[count] given, else NULL): buf = momentum * buf + g / avg, param -= lr * buf;
 * else param -= lr * g / avg. */
int lcrec_rmsprop_step(float *params, float *grads, float *square_avg, float *momentum_buffer, float *grad_avg, int64_t count,
                       const float *clip, int64_t *step, double base_lr, double alpha, double eps, double weight_decay,
                       double momentum, int centered, int schedule, int64_t warmup_steps, int64_t total_steps, float *lr_out,
                       unsigned int *ticket, const unsigned char *skip_flag, void *stream);

/* Dropout masks (nn.Dropout in front of every Linear, index/models/layers.py:17; --dropout_prob of index/main.py).
 * The mask is a FUNCTION of (seed, step, position, element), not a stream of draws, so a captured training step needs no
 * generator state and a test can recompute any mask on the host:
 *   generator  Philox4x32-10 with the standard constants: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl increments
 *              0x9E3779B9 and 0xBB67AE85, 10 rounds
 *   key        (seed low 32 bits, seed high 32 bits)
 *   counter    (q low 32, q high 32, position, (uint32) step), q = flat element index / 4; the four output words belong
 *              to elements 4q .. 4q+3; flat element index = (row_offset + row) * features + col
 *   keep rule  an element is kept iff its word u >= T, T = min(2^32 - 1, floor(p * 2^32)) computed by the caller in double;
 *              kept value = x * s with s = (float)(1.0 / (1.0 - (double)p)) -- one fp32 multiply; dropped value = +0.0f
 * 0 <= p < 1: lcrec_dropout_apply returns LCREC_EINVAL for an s that no such p gives (not finite, below 1, NaN).
 * seed, step: device int64 scalars, read by the kernel -- a replayed hipGraph draws a new mask every step because the
 * optimiser entry points above advance *step, with no new kernel argument.  position: which Dropout module (>= 0).
 * row_offset: global row of this call's row 0 (a rank's shard of a data-parallel batch; 0 otherwise).  features: a positive
 * multiple of 4.  n rows; [n][features] row-major.
 *
 * lcrec_dropout_apply: out = mask * in * s; out may alias in; both 16-byte aligned.  Forward and backward are the same call
 * (the gradient of the dropped tensor's source is g * mask * s).
 * lcrec_dropout_mask: keep_out[n][features] (uint8, 4-byte aligned) = 1 where the element is kept, else 0. */
int lcrec_dropout_apply(const float *in, float *out, int64_t n, int features, uint32_t T, float s, const int64_t *seed,
                        const int64_t *step, int position, int64_t row_offset, void *stream);
int lcrec_dropout_mask(unsigned char *keep_out, int64_t n, int features, uint32_t T, const int64_t *seed, const int64_t *step,
                       int position, int64_t row_offset, void *stream);

/* Embedding files that are not fp32 (the reference takes any float dtype: index/datasets.py:12-18, np.load then
 * torch.FloatTensor): the file's bytes are copied to HBM as they are and converted there, instead of on host threads.
 * dst[i] = (float)src[i] for i < count: fp16 -> fp32 exact, fp64 -> fp32 round-to-nearest-even
 * (overflow -> +-inf, fp32 subnormal results kept, not flushed; NaN stays NaN) -- numpy's astype(float32), bit for bit.
 * Device pointers; src aligned to its element size, dst to 4 bytes -- nothing more is required; src and dst do not overlap.
 * When src and dst reach 16-byte alignment after the same number of leading elements the launch moves 16 bytes per access,
 * otherwise one element per access.
 * count >= 0 (0: no launch).  Enqueued on `stream`, no synchronisation, no allocation, capturable. */
#define LCREC_DTYPE_F16 1
#define LCREC_DTYPE_F64 2
int lcrec_cast_rows(const void *src, int src_dtype, int64_t count, float *dst, void *hip_stream);

/* Which items share an identical index tuple.  Replaces the Python string-set / dict passes of
 * index/trainer.py:139-150 (collision rate) and index/generate_indices.py:18-42
 * (check_collision, get_indices_count, get_collision_item), keeping get_collision_item's order:
 * groups (tuples held by >= 2 items) by first occurrence of the tuple in item order, item ids
 * ascending inside a group.
 *   idx               device [n][L] int64, K host [L] (codes per level; sum of ceil(log2 K) <= 128)
 *                     A code outside its level's range is clamped into it before tuples are compared: v < 0 counts as 0,
 *                     v >= K[l] as K[l] - 1.  So the -1 an index matrix is pre-filled with collides with code 0, and two
 *                     out-of-range codes on the same side of a level are the same code.  idx itself is never written.
 *   members_out       device [n] int64 or NULL: ids of the items of all groups, group after group
 *   group_offsets_out device [n/2+2] int64 or NULL (given together with members_out):
 *                     group g = members_out[off[g] .. off[g+1])
 *                     Only members_out[0 .. counters[2]) and group_offsets_out[0 .. counters[1]] are written.
 *   counters_out      device int64[4]: {distinct tuples, groups, items in groups, largest tuple count};
 *                     entries 1 and 2 are 0 when members_out is NULL;
 *                     collision_rate = (n - counters[0]) / n
 * The argument checks (NULL pointers, n, L, K[l] < 1, more than 128 bits, members without offsets, a workspace smaller than
 * lcrec_collision_groups_workspace(n, L) for n > 0) return before the device is touched.  The workspace may hold anything. */
size_t lcrec_collision_groups_workspace(int64_t n, int L);
int lcrec_collision_groups(const int64_t *idx, int64_t n, int L, const int *K, int64_t *members_out,
                           int64_t *group_offsets_out, int64_t *counters_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/* What lcrec_collision_groups decides on the host for n items of L levels with K[l] codes: the key layout, the bit ranges of its
 * three sorts and where everything lies in the workspace.  lcrec_collision_groups runs by the same function and
 * lcrec_collision_groups_workspace returns its workspace_bytes.  Host only: nothing is launched.  n >= 0 (0 is sized as 1).
 * The key of a tuple is its clamped codes, level 0 in the highest bits, bits[l] bits per level; bit b of the key is bit b of
 * the low word for b < 64, bit b - 64 of the high word above. */
typedef struct {
    int bits[LCREC_MAX_LEVELS];   /* ceil(log2 K[l]) (0 for K = 1); 0 past L */
    int total_bits;               /* their sum, at most 128 */
    int lo_bits;                  /* bits [0, lo_bits) of the low word are sorted first: min(total_bits, 64), 1 for a 0-bit key */
    int hi_bits;                  /* then bits [0, hi_bits) of the high word: total_bits - 64; 0 = no second pass (<= 64 bits) */
    int id_bits;                  /* the last sort, by first item id, over bits [0, id_bits): the smallest b >= 1 with 2^b >= n */
    int64_t stride;               /* bytes from one of the ten n-element arrays to the next: n * 8 rounded up to 256 */
    int64_t temp_bytes;           /* the sorts' and scans' scratch behind the arrays (what rocPRIM asks for on this device) */
    int64_t workspace_bytes;      /* 10 * stride + temp_bytes */
} lcrec_collision_plan;
int lcrec_debug_collision_plan(int64_t n, int L, const int *K, lcrec_collision_plan *out);

/* Nearest-free-code finishing pass: an opt-in step BEYOND the reference.  index/generate_indices.py:107-136 stops after its 20
 * conflict rounds and writes out whatever still collides; this entry follows on from there and gives every item that still shares
 * its tuple a free code of the LAST level.  Only last-level codes change, and only those of the items that move.
 *
 * The rule.  d(i,k) = (xx_i + cc_k) - 2*dot(i,k) with xx, cc and dot each one fp32 fma chain over the dimension ascending from 0:
 * the distance of lcrec_rq_assign, bit for bit.  Wherever two distances are compared a NaN counts as +inf.
 *   1. A bucket is the set of items that share idx[:, :L-1] (L = 1: one bucket of all items).  Only buckets in which some last
 *      code is held by two or more items are touched.
 *   2. Keepers: for each last code k held by >= 2 items of a bucket, the holder with the smallest d(i,k) keeps it; a tie goes to
 *      the lowest item id.  The other holders are movers.
 *   3. Occupied codes: every code held by any item of the bucket, items that collide with nobody included.
 *   4. Movers, in ascending item id: each takes the free code with the smallest d(i,k), the first minimum in code order; that code
 *      is occupied before the next mover looks.  When no code is free, this mover and all later ones of the bucket keep their code
 *      and count as unresolved.
 * So a moved item collides with nobody, the number of colliding items afterwards is exactly `unresolved`, and unresolved is 0
 * whenever no touched bucket has more items than K[L-1].  The result is a function of the inputs alone.
 *
 *   idx             device [n][L] int64, in/out (column L-1 of the movers is rewritten); n < 2^32
 *   K               host [L]; only K[L-1] is used
 *   resid_last      device [n][e] float: the residual entering the last level; e in {16, 32, 64}
 *   codebook_last   device [K[L-1]][e] float; a level lcrec_rq_assign takes (160 KB of LDS)
 *   bucket_members, bucket_offsets   device int64, the layout lcrec_collision_groups emits: bucket b =
 *                   members[off[b] .. off[b+1]), item ids ascending inside a bucket.  Buckets that turn out untouched cost a
 *                   histogram and nothing else, so the groups of idx[:, :L-1] can be passed as they come.  A member whose id is
 *                   outside [0, n) or whose last code is outside [0, K[L-1]) takes no part.
 *   counters_out    device int64[2]: {moved, unresolved}, zeroed by the call
 * n_buckets == 0: no launch, the counters are zeroed.  resid_last and codebook_last 16-byte aligned, the int64 arrays 8-byte.
 * Argument errors are reported before anything is enqueued.  No workspace, no allocation, no synchronisation, capturable. */
int lcrec_finish_nearest_free(int64_t *idx, int64_t n, int L, const int *K, const float *resid_last, int e,
                              const float *codebook_last, const int64_t *bucket_members, const int64_t *bucket_offsets,
                              int64_t n_buckets, int64_t *counters_out, void *stream);

/* Frozen-aware nearest free code: lcrec_finish_nearest_free's pass for a catalogue that GROWS.  Items with id < n_frozen are
 * frozen: they were indexed before, their tuples are the vocabulary a downstream model was trained on, and they never change.  No
 * residual exists for them.  Items n_frozen .. n-1 are new; each keeps its tuple unless that tuple is taken.  Beyond the reference,
 * whose index/generate_indices.py only ever indexes a whole file from scratch.
 *
 * The rule.  d(i,k) is lcrec_finish_nearest_free's distance, bit for bit; wherever two distances are compared a NaN counts as +inf.
 *   1. A bucket is the set of items, frozen and new together, that share idx[:, :L-1] (L = 1: one bucket of all items).  A bucket
 *      is touched only if some last code is held by two or more of its items, at least one of them new.  A bucket with no new item
 *      is never touched, however its frozen items collide.
 *   2. For a last code held by two or more items of a touched bucket: if any holder is frozen, every new holder is a mover.
 *      Otherwise the new holder with the smallest d(i,k) keeps the code, a tie goes to the lowest item id, and the others are movers.
 *   3. Occupied codes: every code held by any item of the bucket, frozen or new.
 *   4. Movers, in ascending item id: each takes the free code with the smallest d(i,k), the first minimum in code order; that code
 *      is occupied from then on.  When no code is free, this mover and all later ones of the bucket keep their code and count as
 *      unresolved.
 * So the frozen rows are bit-identical afterwards; the number of colliding items afterwards (n minus the number of distinct
 * tuples) equals the number colliding among the frozen items alone plus `unresolved`; unresolved is 0 whenever no touched bucket
 * has more items than K[L-1]; and with n_frozen == 0 the result is lcrec_finish_nearest_free's, bit for bit.
 *
 * Arguments as lcrec_finish_nearest_free, except:
 *   n_frozen        0 .. n
 *   resid_last      device [n - n_frozen][e] float: the row of item i is i - n_frozen.  Nothing is read for a frozen id.  May be
 *                   NULL when n_frozen == n.
 *   codebook_last   as there, with 4 more bytes of LDS per code (the frozen holders per code): K[L-1] * (4 e + 24) + 512 bytes
 *                   must fit in 160 KB, which refuses K[L-1] = 1857 .. 1920 at e = 16 and 1075 .. 1088 at e = 32 that
 *                   lcrec_finish_nearest_free takes
 *   bucket_members  item ids ascending inside a bucket (the layout lcrec_collision_groups emits): a bucket whose LAST member is
 *                   frozen holds no new item and is left at once
 * n_buckets == 0 or n_frozen == n: no launch, the counters are zeroed.  Same shape as lcrec_finish_nearest_free: one workgroup
 * per bucket, no workspace, no allocation, no synchronisation, capturable; argument errors are reported before anything is
 * enqueued.  Traced as "extend_nearest_free". */
int lcrec_extend_nearest_free(int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const float *resid_last, int e,
                              const float *codebook_last, const int64_t *bucket_members, const int64_t *bucket_offsets,
                              int64_t n_buckets, int64_t *counters_out, void *stream);

/* Spill to a sibling bucket: what lcrec_finish_nearest_free and lcrec_extend_nearest_free leave unresolved.  Those two passes change
 * last-level codes only, so a bucket (the items sharing all codes but the last) that holds more items than the last level has codes
 * keeps colliding items.  This entry runs after either of them (opt-in, --spill; beyond the reference, as they are): an item with no
 * room in its bucket takes the next-nearest code ONE level up -- what residual quantisation itself suggests -- and the nearest free
 * last-level code there.  The tuple length does not change.  No cascade further up, and the two codes are chosen one after the
 * other, not jointly.
 *
 * Notation: `a` is the second-to-last level L-2, with K2 = K[L-2] codes and codebook C2; the last level L-1 has K1 = K[L-1] codes and
 * codebook C1.  r2_i / r1_i are item i's residuals entering levels L-2 / L-1.  L >= 2.
 *
 * The rule.  d(x, c) = (xx + cc) - 2*dot is lcrec_finish_nearest_free's distance, bit for bit: xx, cc and dot each one fp32 fma
 * chain over the dimension ascending from 0.  Wherever two distances are compared a NaN counts as +inf, and the first minimum in code
 * order wins.  Items with id < n_frozen are frozen (the --extend case); with n_frozen == 0 there are none.
 *   1. Movers.  For each full tuple held by two or more items: if any holder is frozen, every new holder is a mover.  Otherwise the
 *      new holder with the smallest d(r1_i, C1[k]), k the shared last code, keeps the tuple, a tie goes to the lowest id, and the
 *      others are movers.  Frozen items never move; a tuple whose holders are all frozen has no mover.  This is rule 2 of the two
 *      passes above: after either of them it names that pass's unresolved items and nobody else.
 *   2. Super-buckets.  A super-bucket is the set of items, frozen and new, sharing idx[:, :L-2] (L = 2: one super-bucket of all
 *      items).  A cell (a, k) is occupied when any item of the super-bucket holds idx[L-2] = a and idx[L-1] = k.  A super-bucket
 *      without a mover is not touched.
 *   3. Serving.  The movers of a super-bucket are served in ascending item id.  Among the codes a' whose row still has a free cell --
 *      the mover's own row included -- the one with the smallest d(r2_i, C2[a']) is taken.  The residual entering the last level
 *      behind it is computed as lcrec_rq_assign computes it, three fp32 operations per element with c = C2[a'] and r = r2_i:
 *      t = c - r; s = r + t; r' = r - s.  Among the free cells of row a' the k with the smallest d(r', C1[k]) is taken.  Both codes
 *      are written and the cell is occupied from then on.  When no row has a free cell, this mover and all later ones of the
 *      super-bucket keep their tuple and count as unresolved.
 * So columns 0 .. L-3 never change; only movers' rows change; frozen rows are bit-identical; a moved item collides with nobody; the
 * number of colliding items afterwards (n minus the number of distinct tuples) equals the number colliding among the frozen items
 * alone plus `unresolved`; unresolved is 0 whenever no touched super-bucket holds more than K2 * K1 items; and the result is a
 * function of the inputs alone.
 *
 *   idx             device [n][L] int64, in/out (columns L-2 and L-1 of the items that move are rewritten); n < 2^32
 *   n_frozen        0 .. n
 *   K               host [L]; K[L-2] and K[L-1] are used
 *   resid_prev      device [n - n_frozen][e] float: the residual entering level L-2 (L = 2: the latent); the row of item i is
 *   resid_last      i - n_frozen.  resid_last likewise, entering level L-1.  Nothing is read for a frozen id.  e in {16, 32, 64}
 *   codebook_prev   device [K2][e] and [K1][e] float.  Both are staged in LDS with an occupancy bit per cell:
 *   codebook_last       (K2 + K1) * (4 e + 8) + K2 * (4 ceil(K1 / 32) + 4) + 512 bytes
 *                   must fit in 160 KB (256 + 256 codes at e = 64: 144 896); a pair that does not is LCREC_EUNSUPPORTED
 *   tuple_members, tuple_offsets, n_tuple_groups     the groups of the full idx (the shared tuples), and
 *   super_members, super_offsets, n_super_buckets    the groups of idx[:, :L-2] (the super-buckets; L = 2: all items, one group):
 *                   device int64, both in the layout lcrec_collision_groups emits -- group g = members[off[g] .. off[g+1]), item
 *                   ids ascending inside a group.  A member whose id is outside [0, n), or whose code of level L-2 or L-1 is out of
 *                   range, takes no part: it is no holder, occupies no cell and is never written.  A mover is served by the
 *                   super-bucket that lists it.
 *   counters_out    device int64[2]: {moved, unresolved}, zeroed by the call
 *   workspace       device, lcrec_spill_nearest_free_workspace(n) bytes: one mover flag per item (the keeper step needs no more)
 * Two launches: the keepers, one wave per shared tuple, set the flags; then one 256-thread workgroup per super-bucket serves its
 * movers one after the other (two rounds of K2 and K1 distances each).  A two-level model therefore puts ALL items in one
 * workgroup's sequential loop: correct, and slow when many items move (DESIGN.md section 8 has the measurement).
 * No tuple group, no super-bucket or n_frozen == n: no launch, the counters are zeroed.  The float arrays 16-byte aligned, the int64
 * arrays 8-byte.  Argument errors are reported before anything is enqueued and name the argument (workspace too small:
 * LCREC_EWORKSPACE).  No allocation, no synchronisation, capturable.  Traced as "spill_keepers" and "spill_nearest_free". */
size_t lcrec_spill_nearest_free_workspace(int64_t n);
int lcrec_spill_nearest_free(int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const float *resid_prev,
                             const float *resid_last, int e, const float *codebook_prev, const float *codebook_last,
                             const int64_t *tuple_members, const int64_t *tuple_offsets, int64_t n_tuple_groups,
                             const int64_t *super_members, const int64_t *super_offsets, int64_t n_super_buckets,
                             int64_t *counters_out, void *workspace, size_t workspace_bytes, void *stream);

/* Index audit: GIVEN tuples walked through the residual quantiser.  lcrec_finish_nearest_free, lcrec_extend_nearest_free and
 * lcrec_spill_nearest_free -- and the reference's own Sinkhorn rounds -- deliberately give some items a code that is not their
 * nearest one.  This entry says what that cost, per item and level: the distance of the held code, the best distance and the held
 * code's place in the distance ranking.  Beyond the reference, which reports a collision rate and nothing else.
 *
 * The rule.  For item i with latent z_i and held tuple h_i[0 .. L), start with r_0 = z_i and go through the levels l = 0 .. L-1.
 *   1. Distances.  d_l(k) = (xx + cc_k) - 2*dot_k for every code k of level l, xx, cc_k and dot_k each one fp32 fma chain over the
 *      dimension ascending from 0: the distance of lcrec_rq_assign and lcrec_finish_nearest_free, bit for bit.  A NaN distance
 *      counts as +inf wherever distances are compared, and is reported as +inf.
 *   2. Held code.  h = h_i[l] brought into [0, K[l]) by the rule of lcrec_rq_apply_level, decided on the int64 value: below 0
 *      counts as 0, K[l] and above as K[l] - 1.  If the code had to be clamped, bit l of flags_out[i] is set.
 *   3. d_held = d_l(h); best = the first minimum of d_l in code order (what lcrec_rq_assign picks on this residual);
 *      d_best = d_l(best); rank = #{k : d_l(k) < d_l(h)} + #{k < h : d_l(k) == d_l(h)}.  So rank == 0 <=> h == best, and
 *      0 <= rank < K[l].
 *   4. Residual.  It follows the HELD code as lcrec_rq_assign updates it, three fp32 operations per element with c = C_l[h] and
 *      r = r_l: t = c - r; s = r + t; r_{l+1} = r - s.
 * After the last level err = the fp32 fma chain of r_L[j] * r_L[j] over j ascending from 0.
 * Consequences: a tuple written by lcrec_rq_assign / lcrec_encode_assign for the same latent and codebooks has rank 0 and
 * d_held == d_best at every level, and its r_L is that call's last residual, bit for bit; the first level with rank > 0 is where a
 * tuple leaves the greedy path; an item that lcrec_finish_nearest_free moved from its greedy code has rank >= 1 at the last level
 * and rank 0 before it.
 *
 *   z, codebooks, K   as lcrec_rq_assign; e in {16, 32, 64}; 1 <= L <= LCREC_MAX_LEVELS.  Every level lcrec_rq_assign takes is
 *                     taken (the level's rows and cc in LDS: K[l] * (4 e + 20) bytes, less than lcrec_rq_assign needs for it);
 *                     one it refuses is LCREC_EUNSUPPORTED
 *   idx               device int64, read only: item i's held code of level l at idx[i*idx_stride + l]; idx_stride >= L, 0 = L
 *   d_held_out, d_best_out   device [n][L] float
 *   rank_out          device [n][L] int (32-bit)
 *   best_out          device [n][L] int64, or NULL
 *   err_out           device [n] float
 *   resid_out         device [n][e] float, or NULL: r_L
 *   flags_out         device [n] uint32
 *   workspace         device, lcrec_rq_audit_workspace() bytes: the residual between the levels (0 for L == 1)
 * Every output element of rows [0, n) is written by every call.  The float arrays 16-byte aligned, the int64 arrays 8-byte.
 * n == 0: no launch.  One launch per level: one item per lane, the lane sweeps the level's codes once.  No allocation, no host
 * synchronisation, capturable.  Argument errors (LCREC_EINVAL: a NULL pointer, e, L, K[l] < 1, idx_stride < L, misalignment;
 * LCREC_EWORKSPACE) are reported before the device is touched, with a last-error text that names the argument.  Traced as
 * "rq_audit", one bracket per call.  lcrec_rq_audit_workspace returns 0 for arguments lcrec_rq_audit refuses. */
size_t lcrec_rq_audit_workspace(int64_t n, int e, const int *K, int L);
int lcrec_rq_audit(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L,
                   const int64_t *idx, int64_t idx_stride, float *d_held_out, float *d_best_out, int *rank_out,
                   int64_t *best_out, float *err_out, float *resid_out, uint32_t *flags_out,
                   void *workspace, size_t workspace_bytes, void *stream);

/* Beam-search quantiser: the `width` best whole tuples of every item.  lcrec_rq_assign walks the levels greedily -- the nearest
 * code, subtract, move on -- and the finishing, extending and spilling passes only ever move an item off that one tuple.  This
 * entry keeps `width` partial tuples per item, each with its own residual, scores all their children at a level and keeps the
 * `width` best.  Beyond the reference, which is greedy throughout.
 *
 * The rule.  d(r, c_k) = (xx + cc_k) - 2*dot_k, xx, cc_k and dot_k each one fp32 fma chain over the dimension ascending from 0:
 * the distance of lcrec_rq_assign, lcrec_finish_nearest_free and lcrec_rq_audit, bit for bit.  A NaN distance counts as +inf
 * wherever distances are compared, and is reported as +inf.  For item i with latent z_i, width W, levels l = 0 .. L-1:
 *   1. Start with one live beam: residual r = z_i, the empty tuple.  P = 1.
 *   2. At level l every live beam p (in its current order, p = 0 .. P-1) and every code k < K[l] is a candidate with score
 *      s(p, k) = d(r_p, C_l[k]).  The first P' = min(W, P * K[l]) candidates in the order (score ascending, then p ascending,
 *      then k ascending) are the new beams 0 .. P'-1.
 *   3. New beam b from candidate (p, k): its tuple is beam p's tuple with k appended; its residual follows lcrec_rq_assign's three
 *      fp32 operations per element with c = C_l[k] and r = r_p: t = c - r; s = r + t; r' = r - s.
 *   4. After the last level score[b] is the candidate's score at level L-1, err[b] the fp32 fma chain of r_L[j] * r_L[j] over j
 *      ascending from 0 (lcrec_rq_audit's err), and the beams stay in the order of step 2.
 * Consequences: for W = 1 beam 0 is lcrec_rq_assign's tuple, and its err and score are lcrec_rq_audit's err and d_held[:, L-1] of
 * that tuple, bit for bit; for any W, walking beam b's tuple through lcrec_rq_audit reproduces err[b] and score[b] bit for bit; the
 * live beams of an item are pairwise distinct tuples; score is non-decreasing in b; the live count, min(W, K[0] * K[1] * ...) with
 * the product capped at W after every level, depends on W and K alone, and rows b >= live hold -1 in every tuple column and +inf
 * in score, err and resid.  Nothing else is promised: in particular beam 0's err may EXCEED the greedy tuple's (a beam is not
 * monotone; RQVAE.get_indices_beam keeps the greedy tuple for such an item).
 *
 *   z, codebooks, K   as lcrec_rq_assign; e in {16, 32, 64}; 1 <= L <= LCREC_MAX_LEVELS.  Every level lcrec_rq_assign takes is
 *                     taken (the level's rows and cc in LDS: K[l] * (4 e + 20) bytes); one it refuses is LCREC_EUNSUPPORTED
 *   width             1, 2, 4 or 8
 *   tuples_out        device [n][width][L] int64
 *   score_out, err_out   device [n][width] float
 *   resid_out         device [n][width][e] float, or NULL: r_L of every beam
 *   workspace         device, lcrec_rq_beam_workspace() bytes: 0 for L == 1; else the residuals of all beams between the levels,
 *                     [n][width][e] floats rounded up to 256 bytes, once for L == 2 and twice (the levels alternate) for L > 2,
 *                     then the (parent, code) links of the levels before the last, (L-1) * n * width ints rounded up to 256 bytes
 * Every output element of rows [0, n) is written by every call, dead beams included; the workspace may hold anything.  z,
 * codebooks, resid_out and workspace 16-byte aligned, tuples_out 8-byte, score_out and err_out 4-byte.  n == 0: no launch.  One
 * launch per level: an item owns `width` consecutive lanes, one per parent beam; the lane sweeps the level's codes once and keeps
 * its `width` best, the item's lanes merge their lists by lane shuffles, and the last level walks the links back to write the
 * tuples.  No allocation, no host synchronisation, capturable.  Argument errors (LCREC_EINVAL: a NULL pointer, e, L, width,
 * K[l] < 1, misalignment; LCREC_EWORKSPACE) are reported before the device is touched, with a last-error text that names the
 * argument.  Traced as "rq_beam", one bracket per call.  lcrec_rq_beam_workspace returns 0 for arguments lcrec_rq_beam refuses. */
size_t lcrec_rq_beam_workspace(int64_t n, int e, const int *K, int L, int width);
int lcrec_rq_beam(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L, int width,
                  int64_t *tuples_out, float *score_out, float *err_out, float *resid_out,
                  void *workspace, size_t workspace_bytes, void *stream);

/* Beam finishing pass: colliding items move to their next-best WHOLE tuple that nobody holds.  lcrec_finish_nearest_free and the
 * reference's Sinkhorn rounds change the last code of a tuple and lcrec_spill_nearest_free the last two; lcrec_rq_beam lists the
 * `width` best whole tuples of an item, each with its exact quantisation error.  This entry (opt-in, --finish beam; beyond the
 * reference) lets every item that shares its tuple walk down that list.  It is purely combinatorial: it compares tuples and the
 * errors it is given, and computes no distance.
 *
 * The rule.  Items 0 .. n-1 hold the tuples idx[i]; codes are clamped into their level for comparison exactly as
 * lcrec_collision_groups clamps them.  The caller lists the groups of shared tuples in the layout lcrec_collision_groups emits.
 * M = n_members; member position j is item tuple_members[j], with err_held[j], the error of the tuple it holds (lcrec_rq_audit's
 * err), and `width` candidates cand[j][b][0 .. L) with cand_err[j][b], b = 0 .. width-1 in preference order (lcrec_rq_beam's
 * tuples and err of that item's latent).  A candidate with any code outside [0, K[l]) is dead -- lcrec_rq_beam's -1 rows are.
 * Wherever two errors are compared a NaN counts as +inf.
 *   1. Keepers and movers.  In each group the member with the smallest err_held keeps the tuple; a tie goes to the lowest item id.
 *      The others are movers.  A member whose id is outside [0, n) takes no part.
 *   2. Occupied set O.  It starts as the set of tuples held by any of the n items, those that collide with nobody included.
 *   3. Rounds.  Every unplaced mover holds a pointer p, initially 0.  In a round it advances p past every candidate that is dead
 *      or in O -- its own held tuple is in O and is skipped like any other -- and proposes the candidate at p.  A mover whose
 *      pointer reaches `width` is unresolved and keeps its tuple.  Among the movers that propose the same tuple in a round the one
 *      with the smallest cand_err of that candidate wins; a tie goes to the lowest item id.  The winner's row of idx becomes the
 *      candidate, the tuple joins O and the winner is placed; the losers go to the next round with p + 1.  A round is synchronous:
 *      proposals are read against O as it stood when the round began.  Rounds go on until nobody proposes: at most `width` rounds
 *      with a proposal, because a loser's pointer strictly grows.
 * So the rows of non-movers are bit-identical afterwards; a moved item holds a tuple no other item holds; with the groups of idx
 * itself, n minus the number of distinct tuples afterwards equals `unresolved`; with width 1 a mover can only ever take candidate
 * 0; and the result is a function of the inputs alone.
 *
 *   idx             device [n][L] int64, in/out (the whole row of an item that moves is rewritten); n < 2^32
 *   K               host [L]; sum of ceil(log2 K[l]) <= 128 as for lcrec_collision_groups, more is LCREC_EUNSUPPORTED; 1 <= L <= 16
 *   tuple_members, tuple_offsets, n_tuple_groups   device int64, the groups of idx as lcrec_collision_groups emits them: group g =
 *                   members[off[g] .. off[g+1]), item ids ascending inside a group; n_members = off[n_tuple_groups] < 2^32
 *   err_held        device [n_members] float
 *   cand            device [n_members][width][L] int64;  cand_err  device [n_members][width] float
 *   width           1, 2, 4 or 8
 *   choice_out      device [n_members] int: -1 a keeper or a member that takes no part, b >= 0 moved to candidate b, -2 an
 *                   unresolved mover
 *   counters_out    device int64[4]: {movers, moved, unresolved, rounds with at least one proposal}, zeroed by the call
 *   workspace       device, lcrec_finish_beam_workspace() bytes.  With N = max(n, 1), C = max(n_members * width, 1) and every part
 *                   rounded up to 256 bytes: six arrays of N 8-byte words (the held keys: packed, between the two sorts, sorted;
 *                   a low and a high word each), six arrays of C 8-byte words (the candidate keys likewise; the two between the
 *                   sorts then hold every candidate's slot and every slot's winning word), C bytes (the slots' claimed flags),
 *                   max(n_members, 1) ints (the movers' pointers), and behind them what rocPRIM's radix sort asks for max(N, C)
 *                   pairs on this device
 * Launches: pack and sort the held keys, pack and sort the candidate keys, one binary search per candidate in each (is it held;
 * which slot do equal candidates share), one wave per group for the keepers, then the fixed `width` rounds of two launches -- a
 * round without a proposer does nothing -- and one thread for `unresolved`.  The only atomics are min, max and integer add, so
 * the result does not depend on the order of arrival.  n_tuple_groups == 0, n_members == 0 or n == 0: no launch, the counters are
 * zeroed and choice_out is not touched.  The int64 arrays and the workspace 8-byte aligned, the others 4-byte.  The workspace may
 * hold anything on entry.  No allocation, no host synchronisation, capturable; every launch is on `stream`.  Argument errors
 * (LCREC_EINVAL: a NULL pointer, width, L, K[l] < 1, a negative count, misalignment; LCREC_EWORKSPACE) are reported before the device
 * is touched, with a last-error text that names the argument.  Traced as "finish_beam", one bracket per call.
 * lcrec_finish_beam_workspace returns 0 for arguments lcrec_finish_beam refuses. */
size_t lcrec_finish_beam_workspace(int64_t n, int64_t n_members, int L, int width);
int lcrec_finish_beam(int64_t *idx, int64_t n, int L, const int *K, const int64_t *tuple_members, const int64_t *tuple_offsets,
                      int64_t n_tuple_groups, int64_t n_members, const float *err_held, const int64_t *cand,
                      const float *cand_err, int width, int *choice_out, int64_t *counters_out, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Beam finishing pass for a catalogue that grows: lcrec_finish_beam with the first n_frozen items frozen (opt-in, --extend with
 * --extend_finish beam; beyond the reference).  The frozen items are the base file's: their tuples are the vocabulary something
 * downstream was trained on, and no latent, error or candidate exists for them.  A new item that meets a taken tuple walks down its
 * own list of whole tuples, where lcrec_extend_nearest_free can only give it another last code; that pass then runs on what this
 * one counts as unresolved.
 *
 * The rule is lcrec_finish_beam's, with these changes.  Items with id < n_frozen are frozen: they never move, and nothing is read
 * for them from err_held, cand or cand_err -- the rows of a frozen member there may hold anything, and its candidates are dead.
 *   1. Keepers and movers.  Per group, among the members whose id lies in [0, n) (the holders): if any holder is frozen, every new
 *      holder is a mover.  Otherwise the new holder with the smallest err_held keeps the tuple (a NaN counts as +inf, a tie goes to
 *      the lowest item id) and the others are movers.  A group with no new holder has no mover, however its frozen items collide;
 *      a group with fewer than two holders has none.
 *   2. Occupied set O, unchanged: every tuple held by any of the n items, the frozen ones included.
 *   3. Rounds, unchanged: only movers propose.
 * So rows below n_frozen, and the rows of non-movers, are bit-identical afterwards; a moved item holds a tuple no other item holds;
 * with the groups of idx itself, n minus the number of distinct tuples afterwards equals the number colliding among the frozen
 * items alone plus `unresolved`; with n_frozen == 0, idx, choice_out and all four counters are lcrec_finish_beam's, bit for bit.
 *
 * Arguments as lcrec_finish_beam, except:
 *   n_frozen        0 .. n
 *   err_held, cand, cand_err   by member position as there; the positions of frozen members are never read
 *   choice_out      a frozen member gets -1
 *   workspace       lcrec_extend_finish_beam_workspace() bytes: lcrec_finish_beam_workspace's formula
 * n_frozen == n: no launch, the counters are zeroed and choice_out is not touched, as for n_tuple_groups == 0.  Otherwise the same
 * launches on `stream`: the candidate kernels look up the member a candidate belongs to before they look at its row, and the
 * keepers' wave reduction also counts the frozen holders and picks the keeper among the new ones.  The only atomics are min, max
 * and integer add.  No allocation, no host synchronisation, capturable.  Argument errors as lcrec_finish_beam, and n_frozen outside
 * 0 .. n (LCREC_EINVAL), are reported before the device is touched, with a last-error text that names the argument.  Traced as
 * "extend_finish_beam", one bracket per call.  lcrec_extend_finish_beam_workspace returns 0 for arguments the entry refuses. */
size_t lcrec_extend_finish_beam_workspace(int64_t n, int64_t n_members, int L, int width);
int lcrec_extend_finish_beam(int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const int64_t *tuple_members,
                             const int64_t *tuple_offsets, int64_t n_tuple_groups, int64_t n_members, const float *err_held,
                             const int64_t *cand, const float *cand_err, int width, int *choice_out, int64_t *counters_out,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Decode pass: GIVEN tuples back to embeddings, and the reconstruction error of every item.  lcrec_encode_assign goes from an
 * embedding to a tuple and lcrec_rq_audit prices a tuple in latent space; this entry goes the way back -- codes, their sum, the
 * decoder MLP (RQVAE.forward's `out = self.decoder(x_q)`, index/models/rqvae.py:57-66, which the reference runs only inside a
 * training step) -- and compares the result with the item's embedding, which is the quantity the training log prints and a
 * checkpoint is selected on (rqvae.py:74-85).  Beyond the reference, whose index/ stage never turns a tuple back into a vector.
 *
 * The rule.  For item i with held tuple h_i[0 .. L):
 *   1. Held code.  h = h_i[l] brought into [0, K[l]) by the rule of lcrec_rq_apply_level, decided on the int64 value: below 0
 *      counts as 0, K[l] and above as K[l] - 1.  If the code had to be clamped, bit l of flags_out[i] is set.
 *   2. Quantised latent.  q = C_0[h_0], then for l = 1 .. L-1  q = q + C_l[h_l]: one fp32 add per element, levels ascending, and a
 *      plain copy for L == 1.  This is the sum of the CODES.  It is NOT the straight-through sum that lcrec_rq_assign writes to
 *      xq_out, which adds r + (c - r) per level (index/models/vq.py:95): the two differ by rounding only -- by at most
 *      L * 2^-21 * the largest magnitude among residuals, code rows and sums -- but they are not bit-equal: on the greedy tuples of
 *      the test shapes about a third of the elements (30 to 39 %) differ in the last bits.
 *   3. Decoder.  y = layer_{n_layers-1}( ... relu(layer_0(q))): each layer exactly lcrec_linear_forward -- folded eval BatchNorm
 *      where given, ReLU after every layer but the last, the same fp32 fma chains, bit for bit.
 *   4. Error, only when x is given.  d_j = y_j - x_j, one fp32 subtraction.  l1 == 0: err = the fp32 fma chain fma(d_j, d_j, err)
 *      over j ascending from 0, starting at 0.  l1 != 0: err = err + |d_j|, one fp32 add each, j ascending.  One chain per row, so
 *      the result does not depend on any tiling.  The mean of err over all items and columns is the reconstruction loss of
 *      lcrec_recon_loss_grad (which sums in fp64 in another order).
 *
 *   idx         device int64, read only: item i's held code of level l at idx[i*idx_stride + l]; idx_stride >= L, 0 = L
 *   codebooks, K  as lcrec_rq_assign; 1 <= L <= LCREC_MAX_LEVELS.  Nothing is staged in LDS, so any K[l] >= 1 is admitted
 *   dims        host [n_layers+1]: e, hidden sizes ..., the embedding width; dims[0] = e must be 16, 32 or 64
 *   W, b, bn_scale, bn_shift   as lcrec_encode_assign, for the DECODER's layers (b may hold NULL entries: no bias)
 *   xq_out      device [n][e] or NULL: q
 *   out         device [n][dims[n_layers]] or NULL: y.  When it is NULL the last layer writes into the workspace
 *   x           device [n][dims[n_layers]] and err_out device [n]: given together, or both NULL
 *   flags_out   device [n] uint32, or NULL
 * At least one of xq_out, out, err_out must be given; with xq_out alone no layer runs and no workspace is needed.  The float
 * arrays are 16-byte aligned, idx 8-byte, flags_out 4-byte.
 * Items are walked in chunks of lcrec_decode_tuples_chunk_rows() rows.  One pure host function decides the walk and the layout
 * of the workspace (lcrec_debug_decode_tuples_plan, below, reports it): two activation buffers of chunk_rows x the widest layer
 * output -- the last layer's included when want_out == 0 -- and a slab of chunk_rows x e for q, used when xq_out is NULL.  Per
 * chunk, on `stream` only (no context, no pipelines): the gather, the layers, the error kernel.
 * Every layer is validated before the first launch: a width lcrec_linear_forward would refuse is refused here with the same code
 * and a text that names the layer, so no call launches half a pass.  The other argument errors are LCREC_EINVAL / LCREC_EWORKSPACE
 * with a text naming the argument, before the device is touched.  n == 0: no launch.  No allocation, no host synchronisation,
 * capturable.  The workspace may hold anything.  Every requested output element of rows [0, n) is written by every call.
 * Traced as "rq_decode_gather" and "recon_row_error", one bracket per launch (one launch of each per chunk), beside the layers'
 * own labels.  lcrec_decode_tuples_workspace returns 0 for arguments lcrec_decode_tuples refuses. */
size_t lcrec_decode_tuples_workspace(int64_t n, const int *dims, int n_layers, const int *K, int L, int want_out);
/* rows per chunk of the walk described above (a build constant; results do not depend on it) */
int64_t lcrec_decode_tuples_chunk_rows(void);
int lcrec_decode_tuples(const int64_t *idx, int64_t idx_stride, int64_t n, const float *codebooks, const int *K, int L,
                        const int *dims, int n_layers, const float *const *W, const float *const *b,
                        const float *const *bn_scale, const float *const *bn_shift,
                        float *xq_out, float *out, const float *x, int l1, float *err_out, uint32_t *flags_out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Index trie: the prefix trie over the tuples of an index matrix, for the two consumers of an index file -- the exact set of
 * tokens a constrained generation may emit after a prefix, and the items that hold a tuple or its longest prefix.  Beyond the
 * reference, which builds one set of allowed tokens per POSITION (data.py:67-89), so that every combination of codes that occur
 * anywhere at their level is admitted, and which has no way back from a tuple to its items.  Opt-in: nothing else calls it.
 *
 * The three rules.
 *   Build.  Tuples are compared by the key of lcrec_collision_plan: codes clamped as lcrec_collision_groups clamps them (v < 0
 *      counts as 0, v >= K[l] as K[l] - 1), level 0 in the highest bits, at most 128 bits.  Items are sorted by key ascending, then
 *      id ascending.  The nodes of depth d are the distinct clamped prefixes of length d, numbered in key order; depth 0 has the
 *      one node 0.  A node's children are contiguous at the next depth, in ascending code order.
 *   Find.  Longest-prefix descent from (depth 0, node 0): for l = 0 .. depth-1 take c = prefix[b][l]; a code outside [0, K[l])
 *      stops the descent -- query codes are NOT clamped, an out-of-range code is simply absent --, otherwise c is searched among
 *      the node's children, and the descent stops if it is absent.
 *   Mask.  Row b at a live node (0 <= node[b] < counts[depth]) with depth < L may emit { token_ids[c] : c a child code of
 *      node[b] }; with depth == L, or at a dead node, it may emit { eos } (nothing when eos < 0).  Every element of columns [0, V)
 *      outside that set becomes -inf.  Allowed elements are neither read nor written.
 *
 * lcrec_index_trie is a HOST record of DEVICE pointers which the caller allocates; lcrec_index_trie_build fills n, L and K.
 *   order    int64 [n]        item ids by key ascending, then id ascending
 *   counts   int64 [L+1]      counts[d] = nodes of depth d; counts[0] = 1 always
 *   child    int64 [L][n+1]   row d < L: child[d][j] = the index at depth d+1 of node j's first child; child[d][counts[d]] =
 *                             counts[d+1], so node j's children are child[d][j] .. child[d][j+1] - 1
 *   code     int32 [L][n]     row d-1: the last code of every depth-d node
 *   first    int64 [n+1]      leaf j (a node of depth L) holds items order[first[j] .. first[j+1]); first[counts[L]] = n
 * Only those prefixes of each row are written.  n == 0: counts = {1, 0, ...}, child[d][0] = 0 and first[0] = 0 (a row of child then
 * has the one element, and the root has no child).  The int64 arrays are 8-byte aligned, code 4-byte.
 *
 * lcrec_index_trie_build: idx device int64, read only, item i's code of level l at idx[i*idx_stride + l]; idx_stride >= L, 0 = L;
 * K host [L].  Keys are packed and sorted stably by rocPRIM's radix sort, one kernel finds every sorted item's common-prefix length
 * with its predecessor, and per depth a scan of the flags "a node starts here" and one scatter fill the arrays.  The workspace
 * (16-byte aligned, at least lcrec_index_trie_build_workspace(n, L) bytes, 0 for refused arguments) may hold anything.
 *
 * lcrec_index_trie_find: prefix device int64, row b's code of level l at prefix[b*prefix_stride + l]; prefix_stride >= depth,
 * 0 = depth; may be NULL when depth == 0.  node_out device int64 [B], depth_out device int32 [B] or NULL: the node and the depth
 * reached.  With depth_out == NULL, node_out[b] is -1 unless the full depth was reached.  depth == L gives the leaf.
 *
 * lcrec_index_trie_mask_logits: logits device fp32 [B][ld], ld >= V, 4-byte aligned, masked in place; node device int64 [B];
 * token_ids device int32 [K[depth]] or NULL for the identity map (NULL is also what depth == L takes).  Token ids outside [0, V)
 * and columns [V, ld) are never touched.  The kernel only stores: one workgroup per chunk of 4096 columns of a row marks the
 * chunk's allowed tokens in an LDS bitmap and then stores 16 bytes of -inf wherever four columns on a 16-byte boundary are all
 * disallowed, single floats elsewhere and at a row's unaligned head and tail (rows need not start on 16 bytes: odd ld).
 *
 * All four check their arguments before the device is touched: NULL pointers, n < 0, B < 0, L outside 1 .. LCREC_MAX_LEVELS,
 * K[l] < 1, more than 128 key bits, depth outside [0, L], V < 1, ld < V, misalignment (LCREC_EINVAL) and a small workspace
 * (LCREC_EWORKSPACE), each with a text that names the argument.  n == 0 (build) and B == 0 launch nothing.  No allocation, no host
 * synchronisation, capturable.  Traced as "trie_build", "trie_find" and "trie_mask", one bracket per call. */
typedef struct {
    int64_t n;
    int L;
    int K[LCREC_MAX_LEVELS];
    int64_t *order;
    int64_t *counts;
    int64_t *child;
    int *code;
    int64_t *first;
} lcrec_index_trie;
size_t lcrec_index_trie_build_workspace(int64_t n, int L);
int lcrec_index_trie_build(const int64_t *idx, int64_t idx_stride, int64_t n, int L, const int *K, lcrec_index_trie *trie,
                           void *workspace, size_t workspace_bytes, void *stream);
int lcrec_index_trie_find(const lcrec_index_trie *trie, const int64_t *prefix, int64_t prefix_stride, int64_t B, int depth,
                          int64_t *node_out, int *depth_out, void *stream);
int lcrec_index_trie_mask_logits(const lcrec_index_trie *trie, const int64_t *node, int64_t B, int depth, const int *token_ids,
                                 int eos, float *logits, int64_t ld, int64_t V, void *stream);

/* Text of the `.index.json` entries for a run of items (host-side; no device work).  Replaces the
 * per-item Python of index/generate_indices.py:83-92 (token strings "<a_{i}>", "<b_{j}>", ...) and the
 * json.dump of :138-145, whose default separators (", " and ": ") every consumer relies on
 * (data.py:38-89 json.load's the file).  For items first_item .. first_item+n-1 the output is
 *     "<id>": ["<a_i>", "<b_j>", ...], "<id+1>": [...]
 * -- entries joined by ", ", no enclosing braces, no trailing separator, no NUL -- so that
 * "{" + chunk_0 + ", " + chunk_1 + ... + "}" is byte-for-byte json.dump's output for the whole dict.
 *   idx   HOST [n][L] int64 (row-major), 1 <= L <= 26 (prefix letters a..z)
 *   out   HOST buffer of capacity cap bytes; lcrec_index_json_bound(n, L) is always enough
 * Returns the number of bytes written, or a negative LCREC_E* code (LCREC_EWORKSPACE: cap too small). */
int64_t lcrec_index_json_bound(int64_t n, int L);
int64_t lcrec_index_json_format(const int64_t *idx, int64_t n, int L, int64_t first_item, char *out, int64_t cap);

/* The reader of that text (host-side): the strict inverse of "{" + lcrec_index_json_format(items 0 .. n-1) + "}", which is what
 * json.dump with default separators writes for {"0": ["<a_i>", "<b_j>", ...], "1": [...], ...}.  Accepted are exactly the texts
 * the formatter can produce for non-negative codes: keys "0", "1", "2", ... in order, L tokens per item, the prefix letter of
 * each level, codes as decimal digits without sign or leading zeros that fit an int64, ", " and ": " as the only white space,
 * nothing after the closing brace.  So a text that is accepted is reproduced byte for byte by formatting the result.  "{}" gives
 * 0 items.
 *   text      HOST, len bytes, no terminator needed: nothing outside [text, text + len) is read
 *   idx_out   HOST [cap_items][L] int64; rows 0 .. count-1 are written, never a row >= cap_items
 * Returns the item count, or a negative LCREC_E* code with a last-error text that names the byte offset (LCREC_EINVAL: the text
 * is not of that form; LCREC_EWORKSPACE: more than cap_items items; idx_out then holds the items read so far). */
int64_t lcrec_index_json_parse(const char *text, int64_t len, int L, int64_t *idx_out, int64_t cap_items);

/* Kernel tracing (diagnostic; the reference has no tracing on this path -- its only
 * timing is wall-clock per epoch, index/trainer.py:193-195).  While enabled, every
 * kernel this library launches is bracketed by a pair of hipEvents recorded on the
 * launch stream; lcrec_trace_collect() waits for the recorded events, sums elapsed
 * time per kernel and clears the log.  bench.py uses it to price the dominant
 * kernel against its roofline inside the timed region. */
typedef struct {
    const char *kernel;   /* static string, e.g. "linear_fwd_128x128" */
    int64_t launches;
    double total_ms;
} lcrec_trace_entry;
int lcrec_trace_enable(int on);
/* Returns the number of entries written (<= capacity), or a negative LCREC_E* code. */
int lcrec_trace_collect(lcrec_trace_entry *out, int capacity);

/* Debug entries (diagnostic, for the tests: not a path of training or index generation).
 *
 * The batch-sized Sinkhorn solve of lcrec_sinkhorn_assign (a lone group too large for one workgroup) picks one of three
 * solvers by shape; lcrec_debug_sinkhorn_plan reports that choice and its geometry, lcrec_debug_sinkhorn_batch runs it.
 *   form   0 = what lcrec_sinkhorn_assign chooses; 1 = scaling form, eight sets of workgroups that each exchange inside one
 *          XCD; 2 = scaling form, one set, agent-scope exchange; 3 = persistent in-place form; 4 = one launch per iteration.
 *          A forced form that cannot take the shape is LCREC_EUNSUPPORTED, never another form. */
typedef struct {
    int form;                 /* 1 .. 4 as above (never 0) */
    int cpl, rw;              /* columns per lane and rows per wave: the kernel's template arguments (form 4: ceil(K/64), 4) */
    int workgroups;           /* per set */
    int sets;                 /* 1, or 8 for form 1 */
    int rows_per_workgroup;
    int padded_columns;       /* 64 * cpl - K */
    int ragged_wave;          /* the last wave that has rows has fewer than rw */
    int ragged_workgroup;     /* the last workgroup has fewer than rows_per_workgroup */
    int batch_route;          /* whether lcrec_sinkhorn_assign gives a lone group of B rows to this solver at all */
    int64_t workspace_bytes;  /* what lcrec_debug_sinkhorn_batch needs for this shape */
} lcrec_sinkhorn_plan;
/* Host only: nothing is launched, no device is needed. */
int lcrec_debug_sinkhorn_plan(int64_t B, int K, int iters, int form, lcrec_sinkhorn_plan *out);
/* One group of n rows through the batch-sized solver, arguments as for lcrec_sinkhorn_assign, with the same kernels.
 *   runner_out  device int64[n] or NULL: per row the column of the second-largest entry (first one on ties)
 *   ratio_out   device double[n] or NULL (given together with runner_out): second-largest / largest entry of the row
 *   form_ran    host int or NULL: the form whose kernels were launched (0: none)
 * With form = 0 a solver whose launch the runtime refuses (occupancy, LDS attribute) is replaced as in production and
 * form_ran says by which; with a forced form the refusal is LCREC_EUNSUPPORTED. */
int lcrec_debug_sinkhorn_batch(const float *resid, int64_t n, int e, const float *codebook, int K, double epsilon, int iters,
                               int64_t *idx_out, int64_t idx_stride, void *workspace, size_t workspace_bytes,
                               unsigned int *ticket, void *stream, int form, int64_t *runner_out, double *ratio_out,
                               int *form_ran);

/* lcrec_sinkhorn_assign with several groups sorts them into size classes, one launch each: classes 0 .. 3 keep a group's g x K
 * fp64 matrix in LDS (g * K <= 2048 / 4096 / 8192 / 16384 doubles, 256 threads, allocation sized by the class's largest group),
 * class 4 keeps it in a slab of the workspace (1024 threads), and what is left (class 5: more than 4096 rows, or the slab-sized
 * groups of a call in which running them side by side does not pay) goes one group at a time through the batch-sized solver
 * above.  A group that meets a class-3 bound but whose allocation -- (g * K + ((g + 1) & ~1) + K) doubles plus 64 B static --
 * would exceed the 163 840 B a workgroup can have (four rows at K >= 4094, or K = 4 from 4094 rows up) belongs to class 4.
 * lcrec_debug_sinkhorn_groups_plan reports the launches lcrec_sinkhorn_assign makes for a group table: it is the function
 * lcrec_sinkhorn_assign launches by.  Host only: nothing is launched, no device is needed. */
#define LCREC_SK_GROUP_CLASSES 5          /* launches of the one-workgroup-per-group kernel: classes 0 .. 4 */
#define LCREC_SK_CLASS_SLAB 4
#define LCREC_SK_CLASS_BATCH 5
enum { LCREC_SK_TABLE_NONE = 0,           /* no group takes the one-workgroup kernel: no table */
       LCREC_SK_TABLE_ARGUMENT = 1,       /* <= 4 groups: the table travels as a kernel argument */
       LCREC_SK_TABLE_RING = 2,           /* through the context's pinned ring, no host wait */
       LCREC_SK_TABLE_SYNCHRONOUS = 3 };  /* no context: a copy the call waits for */
typedef struct {
    int groups;               /* groups of the class in this call (0: no launch) */
    int maxg;                 /* rows of the largest of them */
    int64_t lds_bytes;        /* dynamic LDS of the launch (class 4: 0) */
    int set_attribute;        /* whether the launch has to raise the kernel's dynamic LDS limit first (more than 48 KB) */
    int threads;              /* 256; class 4: 1024 */
    int table_first;          /* position of the class's first group in the reordered table */
    const char *label;        /* trace label of the launch (static string), NULL without a launch */
} lcrec_sinkhorn_class_plan;
typedef struct {
    lcrec_sinkhorn_class_plan cls[LCREC_SK_GROUP_CLASSES];
    int slab_ok;              /* whether the class-4 groups run side by side (else they take the batch path) */
    int64_t slab_doubles;     /* doubles of the workspace slab */
    int batch_groups;         /* groups routed to the batch-sized solver, one after another */
    int64_t batch_biggest;    /* rows of the largest of them */
    int table_groups;         /* groups in the reordered table (three int64 each: begin, end, slab offset) */
    int transport;            /* LCREC_SK_TABLE_* */
    int fork_mask;            /* bit 0: class 4 on helper stream 0; bit 1: classes 1 .. 3 on helper stream 1 (context only) */
    int64_t workspace_bytes;  /* = lcrec_sinkhorn_assign_workspace */
} lcrec_sinkhorn_groups_plan;
typedef struct {
    int cls;                  /* 0 .. 5; -1 for an empty group */
    int position;             /* in the reordered table (classes in order, offset order inside a class); -1 if not in it */
    int64_t slab_offset;      /* doubles from the slab's start (class 4 in the table), else 0 */
} lcrec_sinkhorn_group_route;
/* routes: NULL, or room for n_groups records. */
int lcrec_debug_sinkhorn_groups_plan(int K, const int64_t *group_offsets, int n_groups, int has_context,
                                     lcrec_sinkhorn_groups_plan *out, lcrec_sinkhorn_group_route *routes);
/* lcrec_sinkhorn_assign with the same arguments and the same launch code, plus what lcrec_debug_sinkhorn_batch adds:
 *   runner_out  device int64[n] or NULL: per row of a group the column of the second-largest entry (first one on ties)
 *   ratio_out   device double[n] or NULL (given together with runner_out): second-largest / largest entry of the row
 * Rows that belong to no group are not written.  With both NULL the kernels launched are lcrec_sinkhorn_assign's own. */
int lcrec_debug_sinkhorn_groups(const float *resid, int64_t n, int e, const float *codebook, int K,
                                const int64_t *group_offsets, int n_groups, double epsilon, int iters,
                                int64_t *idx_out, int64_t idx_stride, void *workspace, size_t workspace_bytes,
                                lcrec_context *ctx, unsigned int *ticket, void *stream, int64_t *runner_out, double *ratio_out);

/* lcrec_rq_assign picks a form of its kernel by shape: the split form (one 64-item tile per 256-thread workgroup, a level's
 * 32-code blocks dealt over its four waves) or one tile per wave, 256 or 512 threads, a grid, and a greedy packing of consecutive
 * levels into launches whose codebooks fit in LDS.  lcrec_debug_rq_assign_plan reports that choice and its geometry,
 * lcrec_debug_rq_assign runs it.
 *   force_split    -1 = what lcrec_rq_assign chooses; 0 = one tile per wave; 1 = the split form (256 threads)
 *   force_threads  0 = what lcrec_rq_assign chooses; 256 or 512
 *   force_grid     0 = what lcrec_rq_assign chooses; else 1 .. that choice for the form (fewer workgroups: more trips of the
 *                  tile loop at a small n)
 * A forced form that cannot take the shape is LCREC_EUNSUPPORTED, never another form: 512 threads with e = 64 or with the split
 * form, the split form when its hand-over buffers push a level out of LDS, a grid out of range. */
typedef struct {
    int split;                /* 1 = split form */
    int threads;              /* 256 or 512 */
    int grid;                 /* workgroups of every launch */
    int64_t tiles;            /* ceil(n / 64) */
    int64_t trips_max, trips_min;   /* trips of the tile loop: per workgroup in the split form, per wave otherwise (0: a wave idles) */
    int launches;
    /* per launch i < launches: levels l0[i] .. l1[i]-1, their staged (padded) LDS rows, the launch's dynamic LDS bytes */
    int l0[LCREC_MAX_LEVELS], l1[LCREC_MAX_LEVELS], rows[LCREC_MAX_LEVELS];
    int64_t lds_bytes[LCREC_MAX_LEVELS];
    int row_off[LCREC_MAX_LEVELS];          /* per level: its first LDS row within its launch */
    /* per level, split form only (else 0): 32-code blocks in a wave's share, and waves whose share is empty */
    int blocks_per_wave[LCREC_MAX_LEVELS], idle_waves[LCREC_MAX_LEVELS];
    /* split form, some launch runs an odd number of levels and some workgroup makes more than one trip: the last level of a
     * tile and the first of the next are then consecutive uses of the hand-over buffers with the same level parity */
    int handover_reuse;
} lcrec_rq_plan;
/* Host only: nothing is launched, no device is needed.  n >= 1. */
int lcrec_debug_rq_assign_plan(int64_t n, int e, const int *K, int L, int force_split, int force_threads, int force_grid,
                               lcrec_rq_plan *out);
/* lcrec_rq_assign with the three forcing arguments: the same launcher, plan and kernels. */
int lcrec_debug_rq_assign(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L,
                          int64_t *idx_out, int64_t idx_stride, float *xq_out, int xq_accumulate, double *sse_out,
                          float *resid_out, float *margin_out, uint32_t *neartie_out, float tie_tau,
                          void *workspace, size_t workspace_bytes, unsigned int *ticket, void *stream,
                          int force_split, int force_threads, int force_grid);

/* lcrec_encode_assign walks its n rows in chunks; one pure host function decides the walk and the layout of the workspace, and
 * the workspace query, the launch code and the export below all go through it:
 *   - chunk c covers rows c * chunk_rows .. and every chunk but the last has chunk_rows rows;
 *   - it runs on pipeline c % pipelines (0: the caller's stream, 1: the context's first helper stream), the pipelines in use
 *     being min(asked for, chunks, LCREC_ENC_PIPES_MAX), at least 1;
 *   - layer l of the chunk writes activation buffer first_act + (l & 1) -- every pipeline ping-pongs between two buffers of its
 *     own, each act_bytes = chunk_rows x widest hidden width floats rounded up to 256 B -- and the last layer writes rows
 *     row0 .. row0 + rows of the latent matrix, which is latent_out or, when that is NULL, the slab at latent_offset;
 *   - one lcrec_rq_assign over all n rows follows, with the rq_bytes at rq_offset as its workspace.
 * The workspace always has room for LCREC_ENC_PIPES_MAX pipelines and for the latent slab, used or not, so its size depends on
 * the shapes and the chunk size alone.  chunk_rows: 0 = the built-in lcrec_encode_assign_chunk_rows(); any positive value is
 * admitted (results do not depend on it); a batch shorter than a chunk is one chunk of n rows. */
#define LCREC_ENC_PIPES_MAX 2
#define LCREC_ENC_ACT_BUFFERS 4           /* 2 * LCREC_ENC_PIPES_MAX */
typedef struct {
    int64_t n;                /* rows of the call */
    int64_t chunk_rows;       /* the chunk size in effect: min(asked for, max(n, 1)) */
    int64_t n_chunks;         /* ceil(n / chunk_rows) */
    int pipelines;            /* pipelines in use */
    int64_t act_bytes;        /* one activation buffer */
    int64_t act_offset[LCREC_ENC_ACT_BUFFERS];   /* byte offsets into the workspace: pipeline p owns buffers 2p and 2p + 1 */
    int64_t latent_offset, latent_bytes;         /* the slab for [n][e] latents (used when latent_out is NULL) */
    int64_t rq_offset, rq_bytes;                 /* lcrec_rq_assign's workspace for n rows */
    int64_t total_bytes;      /* = lcrec_encode_assign_workspace */
} lcrec_encode_plan;
typedef struct {
    int64_t row0, rows;
    int pipeline;
    int first_act;            /* index into act_offset of the buffer the chunk's first layer writes (when it is not the last) */
} lcrec_encode_chunk;
/* Host only: nothing is launched, no device is needed.  pipelines: 1 .. LCREC_ENC_PIPES_MAX, what the context would be set to.
 * plan_out is required; chunks_out is NULL (capacity is then not read), or room for `capacity` >= n_chunks records.  Returns
 * LCREC_OK or the code lcrec_encode_assign refuses the arguments with (LCREC_EINVAL too for a capacity that is too small). */
int lcrec_debug_encode_assign_plan(int64_t n, const int *dims, int n_layers, const int *K, int L, int64_t chunk_rows, int pipelines,
                                   lcrec_encode_plan *plan_out, lcrec_encode_chunk *chunks_out, int64_t capacity);
/* lcrec_encode_assign_workspace for a chunk size (0 for refused arguments, chunk_rows < 0 among them). */
size_t lcrec_debug_encode_assign_workspace(int64_t n, const int *dims, int n_layers, const int *K, int L, int64_t chunk_rows);
/* lcrec_encode_assign with the chunk size as an argument: the same launch code, plan and kernels. */
int lcrec_debug_encode_assign(const float *x, int64_t n, const int *dims, int n_layers,
                              const float *const *W, const float *const *b,
                              const float *const *bn_scale, const float *const *bn_shift,
                              const float *codebooks, const int *K, int L, int64_t *idx_out,
                              float *latent_out, float *xq_out, double *sse_out,
                              float *margin_out, uint32_t *neartie_out, float tie_tau,
                              void *workspace, size_t workspace_bytes, lcrec_context *ctx, void *stream, int64_t chunk_rows);

/* lcrec_decode_tuples walks its n rows in chunks; one pure host function decides the walk and the layout of the workspace, and
 * the workspace queries, the launch code and the export below all go through it:
 *   - chunk c covers rows c * chunk_rows .. and every chunk but the last has chunk_rows rows (the last: last_chunk_rows);
 *   - the gather writes the chunk's q to rows c * chunk_rows .. of xq_out or, when that is NULL, to the slab at q_offset;
 *   - layer l of the chunk writes the activation buffer at act_offset[l & 1], each act_bytes = chunk_rows x `widest` floats rounded
 *     up to 256 B, `widest` being the widest output of the layers that write there: every layer but the last, and the last one
 *     too when want_out == 0; with want_out != 0 the last layer writes the chunk's rows of `out`;
 *   - the error kernel reads the last layer's output where it was written.
 * The q slab is part of the workspace whether xq_out is given or not, so the size depends on the shapes, want_out and the chunk
 * size alone.  chunk_rows: 0 = the built-in lcrec_decode_tuples_chunk_rows(); any positive value is admitted (results do not
 * depend on it); a batch shorter than a chunk is one chunk of n rows. */
typedef struct {
    int64_t n;                /* rows of the call */
    int64_t chunk_rows;       /* the chunk size in effect: min(asked for, max(n, 1)) */
    int64_t n_chunks;         /* ceil(n / chunk_rows) */
    int64_t last_chunk_rows;  /* rows of the last chunk (0 for n == 0) */
    int widest;               /* floats per row of an activation buffer (0: no layer writes there) */
    int64_t act_bytes;        /* one activation buffer */
    int64_t act_offset[2];    /* byte offsets into the workspace */
    int64_t q_offset, q_bytes;   /* the slab for [chunk_rows][e] quantised latents (used when xq_out is NULL) */
    int64_t total_bytes;      /* = lcrec_decode_tuples_workspace */
} lcrec_decode_plan;
/* Host only: nothing is launched, no device is needed.  Returns LCREC_OK or the code lcrec_decode_tuples refuses the shapes with. */
int lcrec_debug_decode_tuples_plan(int64_t n, const int *dims, int n_layers, const int *K, int L, int want_out, int64_t chunk_rows,
                                   lcrec_decode_plan *plan_out);
/* lcrec_decode_tuples_workspace for a chunk size (0 for refused arguments, chunk_rows < 0 among them). */
size_t lcrec_debug_decode_tuples_workspace(int64_t n, const int *dims, int n_layers, const int *K, int L, int want_out,
                                           int64_t chunk_rows);
/* lcrec_decode_tuples with the chunk size as an argument: the same launch code, plan and kernels. */
int lcrec_debug_decode_tuples(const int64_t *idx, int64_t idx_stride, int64_t n, const float *codebooks, const int *K, int L,
                              const int *dims, int n_layers, const float *const *W, const float *const *b,
                              const float *const *bn_scale, const float *const *bn_shift,
                              float *xq_out, float *out, const float *x, int l1, float *err_out, uint32_t *flags_out,
                              void *workspace, size_t workspace_bytes, void *stream, int64_t chunk_rows);

/* The BatchNorm strip calls pick a kernel form by shape and alignment; lcrec_debug_bn_plan reports it.  Host only: nothing is
 * launched.  call: LCREC_BN_*; aligned: whether every pointer the call would be given sits on 16 bytes; 1 <= n <= 2^20. */
enum { LCREC_BN_FORWARD = 0, LCREC_BN_BACKWARD, LCREC_BN_STATS, LCREC_BN_BACKWARD_REDUCE, LCREC_BN_BACKWARD_APPLY };
typedef struct {
    int float4;               /* 1 = float4 strips (features % 4 == 0, aligned, <= 8 rows per lane, n * features < 2^29), 0 = dword */
    int cols;                 /* strip width in columns: 4, 8 or 16 (float4); 8, 16 or 32 (dword) */
    int rows_per_lane;        /* float4: 1, 2, 4 or 8 (the kernel's template argument); dword: 0 (a loop over the rows) */
    int cached;               /* dword forward / backward: the lane's rows stay in registers between the passes (1025 <= n <= 32 rows per lane) */
    int grid;                 /* workgroups, one per strip: ceil(features / cols) */
    int xcd_order;            /* workgroup b takes strip (b % 8) * (grid / 8) + b / 8, not strip b (grid a multiple of 8) */
} lcrec_bn_plan;
int lcrec_debug_bn_plan(int call, int64_t n, int features, int aligned, lcrec_bn_plan *out);

/* The reduction and gradient tail of a training step: the launch each call below picks for its size and alignment;
 * lcrec_debug_step_tail_plan reports it, and the launchers launch by the same function.  Host only: nothing is launched.
 *   call        LCREC_TAIL_*
 *   n_or_count  rows n (relu_bias_backward, quantizer_input_grad_bias, rq_apply_level, code_stats*), or elements `count`
 *               (recon_loss_grad, grad_norm_clip); >= 1
 *   width       features (relu_bias_backward), e (quantizer_input_grad_bias, rq_apply_level, code_stats*); unused for the two
 *               flat reductions
 *   aligned     whether every array of the call sits on 16 bytes (read by the two flat reductions only)
 *   out->K      IN, the two code_stats calls only: the codebook size (code_stats_levels: the largest of the levels') */
enum { LCREC_TAIL_RELU_BIAS_BACKWARD = 0, LCREC_TAIL_RECON_LOSS_GRAD, LCREC_TAIL_GRAD_NORM_CLIP, LCREC_TAIL_QUANTIZER_INPUT_GRAD_BIAS,
       LCREC_TAIL_RQ_APPLY_LEVEL, LCREC_TAIL_CODE_STATS, LCREC_TAIL_CODE_STATS_LEVELS };
enum {
    LCREC_TAILK_STRIP = 0,          /* relu_bias_backward_kernel<cols>: one 1024-thread workgroup per strip of columns */
    LCREC_TAILK_REDUCE,             /* recon_loss_grad_kernel / sumsq_kernel: fp64 partial per 1024-thread workgroup */
    LCREC_TAILK_QGB_ONE,            /* quantizer_input_grad_bias_kernel: one workgroup (e 16 / 32 / 64, n * e <= 65536) */
    LCREC_TAILK_QG_TWO,             /* quantizer_input_grad_kernel, then the strip kernel over its output */
    LCREC_TAILK_APPLY_LEVEL,        /* apply_level_kernel */
    LCREC_TAILK_CS_SORTED,          /* code_stats_sorted_kernel: counting sort in LDS (n <= 8192, K <= 1024) */
    LCREC_TAILK_CS_STREAMING,       /* code_stats_kernel: every thread scans all items */
    LCREC_TAILK_CS_LEVELS,          /* code_stats_levels_kernel: the sorted form of all levels in one launch, gridDim.y = L */
    LCREC_TAILK_CS_PER_LEVEL        /* code_stats_levels falls back to lcrec_code_stats (+ lcrec_codebook_grad) level by level */
};
typedef struct {
    int K;                    /* IN (see above); 0 otherwise */
    int family;               /* LCREC_TAILK_* */
    int grid;                 /* workgroups of the (first) launch; gridDim.x.  CS_PER_LEVEL: 0, see LCREC_TAIL_CODE_STATS */
    int grid_sse;             /* rq_apply_level given sse_out: the partial sums' grouping follows the grid, at most 256; else 0 */
    int cols;                 /* STRIP: strip width in columns (8, 16 or 32); else 0 */
    int xcd_order;            /* STRIP: workgroup b takes strip (b % 8) * (grid / 8) + b / 8 (grid a multiple of 8) */
    int vec16;                /* REDUCE: the 16-byte loop runs (aligned); APPLY_LEVEL and the CS forms: always 16-byte rows */
    int second_launch;        /* a launch follows the first: REDUCE and APPLY_LEVEL's sse when the call is given no ticket (the
                               * finishing kernel); QG_TWO and CS_PER_LEVEL always */
    int64_t tail;             /* elements outside the main loop.  REDUCE: read by scalars, count % 4 with vec16, else all `count`;
                               * STRIP: rows past the last whole block of 8 x (1024 / cols) rows, taken one row per lane and
                               * trip (a row group whose eighth row is still below n takes them in one more unrolled trip);
                               * QGB_ONE: rows past the last whole block of 4 x (1024 / e) rows, whose missing rows are clamped
                               * loads; else 0 */
} lcrec_step_tail_plan;
int lcrec_debug_step_tail_plan(int call, int64_t n_or_count, int width, int aligned, lcrec_step_tail_plan *out);

/* The launch of the four optimiser entry points (lcrec_adamw_step .. lcrec_rmsprop_step: one kernel, one launcher) for
 * `count` elements; the launcher takes its grid from the same function.  Host only: nothing is launched.
 *   aligned     whether params, grads and every state buffer the rule uses sit on 16 bytes (one that does not sends
 *               every element through the scalar loop)
 *   has_ticket  whether the call is given a ticket
 * A lane is one of the workgroups x 1024 threads; both loops stride by that many, so lane t makes
 * ceil((items - t) / lanes) trips over a loop's items (0 when t >= items): the first lane the most, the last the fewest. */
typedef struct {
    int workgroups;           /* gridDim.x: ceil(count / 8192), at most 256 */
    int second_launch;        /* no ticket: a one-thread launch advances *step (and momentum_ready) */
    int64_t quads;            /* float4 items of the 16-byte loop: count / 4 when aligned, else 0 */
    int64_t scalars;          /* elements of the scalar loop: count % 4 when aligned, else count */
    int64_t quad_trips_max, quad_trips_min;       /* trips of the 16-byte loop: the first lane's, the last lane's */
    int64_t scalar_trips_max, scalar_trips_min;   /* the same for the scalar loop */
} lcrec_optim_plan;
int lcrec_debug_optim_plan(int64_t count, int aligned, int has_ticket, lcrec_optim_plan *out);

/* The launches of lcrec_linear_forward, lcrec_linear_backward, lcrec_linear_backward_weights and lcrec_linear_bn_forward
 * (csrc/gemm_f32.hip): each entry point decides its launches with one pure host function; the launch code launches by it and the
 * debug exports below report it.  Host only: nothing is launched, no device is needed.  One lcrec_gemm_launch per kernel launch.
 * The debug plan records are not part of the versioned surface: fields are added at the end without a new LCREC_ABI_VERSION. */
enum { LCREC_GEMMK_TILE_BODY = 0,   /* linear_tile_body: linear_fwd_kernel / linear_train_fwd_kernel / linear_dw_grouped_kernel */
       LCREC_GEMMK_32x64,           /* linear_s16_kernel */
       LCREC_GEMMK_REDUCER,         /* splitk_reduce_kernel / splitk_reduce_grouped_kernel */
       LCREC_GEMMK_PP };            /* the ping-pong kernels: linear_fwd_pp2_kernel / linear_fwd_pp3_kernel (`form`) */
enum { LCREC_GEMMR_DX = 0, LCREC_GEMMR_DW, LCREC_GEMMR_REDUCE, LCREC_GEMMR_FORWARD };
typedef struct {
    const char *label;        /* the trace label the launch is counted under (a reducer runs inside its product's bracket) */
    int role;                 /* LCREC_GEMMR_* */
    int family;               /* LCREC_GEMMK_* */
    int tile_rows, tile_cols; /* the workgroup tile (reducer: 0) */
    int fast;                 /* buffer-load staging (K % 32 == 0 or k-major operands), not the guarded loads */
    int a_kmajor, w_kmajor;   /* the TA / TB template switches */
    int pro;                  /* 0; 1: scale / shift / clamp on the row-major A operand; 2: on the k-major W operand */
    int stats;                /* batch statistics in the epilogue */
    int register_buffered;    /* the tile body's DB form (ring of four register sets, k_tile_rb); the 32x64 kernel: always 1 */
    int64_t m;                /* the product's output is [m][n], contracted over k */
    int n, k;
    int k_tiles;              /* ceil(k / 32) */
    int runs;                 /* S: K-runs (gridDim.y); reducer: the partial products it adds */
    int k_tiles_per_run;      /* K-tiles of every run but the last */
    int k_tiles_last_run;
    int last_k_valid;         /* valid k of the last K-tile (32: not ragged) */
    int tiles, virtual_tiles; /* output tiles, and the numbering's extent (row panels padded to the 8 XCDs: the rest are holes) */
    int workgroups;           /* grid size, all K-runs included (reducer: ceil(total4 / 256)) */
    int wg_start;             /* grouped launches: the problem's first workgroup in the shared grid */
    int last_panel_rows;      /* valid rows of the last row panel */
    int last_tile_cols;       /* valid columns of the last column tile */
    int vector_stores;        /* n % 4 == 0: 16-byte stores */
    int chunk_row_tiles;      /* stats: row tiles per merge chunk (CH); else 0 */
    int chunks;               /* stats: merge chunks, ceil(row tiles / CH); else 0 */
    int64_t total4;           /* reducer: float4 sums */
    /* lcrec_linear_forward only (else 0) */
    int64_t row0;             /* the first row of the call this launch covers: rows row0 .. row0 + m */
    int form;                 /* 0: not a ping-pong launch, 2: per-tile (linear_fwd_pp2_kernel), 3: persistent (linear_fwd_pp3_kernel) */
    /* persistent form only (else 0) */
    int steady_iterations;    /* STEADY iterations per tile */
    int list_min, list_max;   /* shortest and longest tile list of a workgroup */
    int empty_workgroups;     /* workgroups with no tile */
    int single_tile_workgroups; /* ... and with exactly one */
    int ragged_handed_over;   /* tiles of a ragged last row panel that are NOT the last of their list (their partial row count goes
                               * through the hand-over to the next tile's K loop instead of through finish()) */
} lcrec_gemm_launch;
/* The launches lcrec_linear_forward makes for [n][in_dim] -> [n][out_dim] on a device of `cus` compute units, in order, into
 * out[0 .. capacity), capacity >= 4.  Returns the count (0 for n = 0) or a negative code for a shape lcrec_linear_forward refuses;
 * unlike the three below it then leaves lcrec_last_error() as it was. */
int lcrec_debug_linear_forward_plan(int64_t n, int in_dim, int out_dim, int cus, lcrec_gemm_launch *out, int capacity);
/* out[0 .. capacity), capacity >= 3: the dX launch (want_gx), the dW launch and its reducer (want_gw, S > 1), in launch order.
 * Returns the count or a negative code for a shape lcrec_linear_backward refuses. */
int lcrec_debug_linear_backward_plan(int64_t n, int in_dim, int out_dim, int want_gx, int want_gw, lcrec_gemm_launch *out, int capacity);
/* out[p] for problem p < count, every one a part of ONE launch of grid_out[0] workgroups, then one record per problem with
 * S > 1, in problem order: its part of the grouped reducer's launch of grid_out[1] workgroups (0: not launched).  capacity >=
 * 2 * count.  Of the problems only sizes, `splits` and whether x_scale / x_shift are given are read.  Returns the number of
 * records or a negative code. */
int lcrec_debug_linear_backward_weights_plan(const lcrec_dw_problem *problems, int count, lcrec_gemm_launch *out, int capacity,
                                             int *grid_out);
/* The one launch of lcrec_linear_bn_forward with an input fold (pro) and / or statistics (stats).  Returns 1, 0 when neither is
 * asked for (the call is lcrec_linear_forward's then), or a negative code for a refused shape. */
int lcrec_debug_linear_bn_forward_plan(int64_t n, int in_dim, int out_dim, int pro, int stats, lcrec_gemm_launch *out);

#ifdef __cplusplus
}
#endif
#endif /* LCREC_H */
