/* mobocmf_hip.h -- C-ABI of the MI355X (gfx950) MFDGP hot path.
 *
 * Drop-in boundary for the variational multi-fidelity deep-GP layer + ELBO of fernandezdaniel/MOBOCMF.
 * The reference has no FFI of its own (it is pure Python on GPyTorch); these entry points replace the
 * arithmetic that the reference reaches through the following call sites (paths under /root/reference):
 *
 *   mobocmf_layer_forward / _backward   mobocmf/layers/mfdgp_hidden_layer.py:232-243 (prior over cat[Z,X]),
 *                                       :286 -> gpytorch UnwhitenedVariationalStrategy.forward (Gram, Cholesky,
 *                                       triangular solves, predictive moments) and kl_divergence(); backward =
 *                                       what torch autograd does for blackbox_mfdgp_fitter.py:168
 *   mobocmf_propagate_forward/_backward mobocmf/layers/mfdgp_hidden_layer.py:263-274 (hidden-sample propagation)
 *   mobocmf_elbo_data_forward/_backward mobocmf/mlls/variational_elbo_mf.py:31-35 + GaussianLikelihood.expected_log_prob
 *   mobocmf_acq_moments_forward/_backward  mobocmf/models/mfdgp.py:258-260 (moments over the S samples)
 *   mobocmf_jes_forward                 mobocmf/acquisition_functions/JESMOC_MFDGP.py:52
 *   mobocmf_predictive_covariance       eval branch of the variational strategy: K_nn - K_nm K_mm^-1 K_mn + C^T C
 *                                       (the full covariance GPyTorch materialises in .eval(), JESMOC_MFDGP.py:42)
 *   mobocmf_adam_step                   torch.optim.Adam.step at blackbox_mfdgp_fitter.py:169
 *
 * Conventions: all pointers are DEVICE pointers to row-major float64 unless stated; sizes are explicit;
 * every function enqueues work on `stream` and returns immediately (no allocation, no free, no host sync;
 * re-entrant, one process per GPU).  The library holds NO mutable state between calls: every kernel-selection knob
 * travels with the call in a `mobocmf_tuning` (a pointer in the layer descriptor, or an argument of the standalone
 * product entry points; NULL = the compiled-in defaults), block-activity arrays and probe events are explicit arguments,
 * and the workspace-size queries take the same descriptor / tuning as the launch they size for.  Two host threads with
 * different tunings on different streams do not interact.  (One write-once bit per kernel instantiation and device
 * remembers that the kernel's dynamic-LDS attribute was set on that device.)  Return value: MOBOCMF_OK or an error
 * code; a non-positive-definite K_mm is reported through the device word `info` (0 = OK, k>0 = pivot k
 * failed), mirroring LAPACK potrf / torch.linalg.cholesky_ex, so the caller may retry with more jitter
 * (gpytorch psd_safe_cholesky semantics) without a sync on the fast path.
 *
 * The Python binding (mobocmf_amd/_lib.py) is DERIVED from this file at import, and reads three declaration forms only:
 *   constants   `#define MOBOCMF_X <integer expression>` (literals, ( ) + * <<, earlier MOBOCMF_ names) and the anonymous enum;
 *   structs     `typedef struct [tag] { ... } name;` with fields of int32_t / uint32_t / int64_t / uint64_t / double / size_t,
 *               pointers, earlier structs of this file, and 1- or 2-dimensional arrays of these with constant bounds;
 *   functions   `int mobocmf_name(args);` with scalars of those types, pointers and mobocmf_stream_t.
 * Anything else of these kinds (a bitfield, a function pointer, a float, a function-like macro) makes the import raise.
 */
#ifndef MOBOCMF_HIP_H
#define MOBOCMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mobocmf_stream_t; /* hipStream_t */

#define MOBOCMF_MAX_D 32    /* input dimensions a layer accepts (x columns; the Gram kernels keep a row in registers) */
#define MOBOCMF_MAX_XDIV 48 /* sample replicas per base row (num_samples_for_acquisition / _for_training) */

enum {
    MOBOCMF_OK = 0,
    MOBOCMF_BAD_ARG = 1,
    MOBOCMF_WORKSPACE_TOO_SMALL = 2,
    MOBOCMF_HIP_ERROR = 3,
    MOBOCMF_NOT_PD = 4, /* only returned by mobocmf_check_info (host-side, synchronising) */
    MOBOCMF_BAD_ARCH = 5
};

/* Kernel-selection knobs of one call.  Fill with mobocmf_tuning_init() (compiled-in defaults, struct_size), change what is
 * needed, and pass the pointer with the call; NULL everywhere means the defaults.  Knobs never change results beyond
 * summation order; they exist for size sweeps, A/B timing and the parity tests.  A workspace-size query and the launch it
 * sizes for must be given the same values (syrk_workgroups changes the slab count, tile_rows the partial-row count): the
 * launches re-derive their layout from the tuning they receive and return MOBOCMF_WORKSPACE_TOO_SMALL on a mismatch. */
typedef struct mobocmf_tuning {
    uint32_t struct_size;    /* sizeof(mobocmf_tuning) of the caller (versioning; set by mobocmf_tuning_init) */
    int32_t small_gemm_max;  /* largest dimension of an M x M product on the small-operand kernel (default 384, <= 512) */
    int32_t small_panel_max; /* largest K of an M x N' panel product on the whole-block panel kernel (default 512, <= 512) */
    int32_t tile_rows;       /* tile height of the M x N' panel products: 0 = by shape (default) | 64 | 128 */
    int32_t pair_mode;       /* one workgroup does the row blocks (p, n-1-p) of a triangular product: 0 auto | 1 never | 2 always */
    int32_t mid_gemm_max;    /* largest dimension of a plain M x M product on the mid-size kernel (default 1024; 0 = off) */
    int32_t mid_gemm_waves;  /* its form: 32 (default) = 32 x 64 tiles, 64-k stages | 8 | 4 = 64 x 64 tiles on 8 / 4 wavefronts */
    int32_t syrk_workgroups; /* workgroups a k-sliced weighted syrk may occupy: 0 = by shape (default) | 16..4096 */
    int32_t sparse_backward; /* 1 (default): a layer backward skips 128-column blocks whose upstream gradients are all
                              * exactly zero (the rows of other fidelities, variational_elbo_mf.py:33-38) -- found on the
                              * device, same numbers; 0: the dense backward (A/B timing, parity tests) */
    int32_t potrf_cols;      /* the blocked Cholesky: 0 (default) = all 64-column steps in ONE launch where it applies (128 < M <= 1024;
                              * panel and trailing-update workgroups resident together), the four-column panel kernel elsewhere |
                              * 4 | 1 = one launch pair per 64 columns, 4 / 1 columns per hand-over of its panel kernel */
} mobocmf_tuning;
int mobocmf_tuning_init(mobocmf_tuning* t);

/* One variational GP layer.
 * kind 0 (first layer):  k = alpha * RBF_ard(x, x')                              hyp = [alpha, ls[0..d)]
 * kind 1 (layer >= 1):   k = a1*RBF(x,x';ls1) * (nu*f*f' + af*RBF(f,f';lsf)) + a2*RBF(x,x';ls2)
 *                        hyp = [a1, af, nu, a2, lsf, ls1[0..d), ls2[0..d)]
 * The data matrix X~ = [x[n / xdiv], f[n]] is never materialised: row n of the layer input uses row n/xdiv of
 * `x` (S-fold sample replication, mfdgp.py:248 / SURVEY F7) and f[n] (kind 1 only).  Inducing inputs Z~ = [Zx, zf].
 */
typedef struct {
    int32_t kind;    /* 0 | 1 */
    int32_t d;       /* columns of x and Zx, 1..MOBOCMF_MAX_D */
    int32_t M;       /* inducing points */
    int32_t xdiv;    /* 1..MOBOCMF_MAX_XDIV */
    int64_t Np;      /* rows through the layer (N'), Np % xdiv == 0 */
    int32_t branch;  /* 0: training branch (clamp(k_nn - q, 0)); 1: eval branch (no clamp) */
    int32_t want_dx; /* backward also returns d/dx (acquisition optimisation) */
    double jitter;   /* added to diag(K_mm); gpytorch variational_cholesky_jitter = 1e-6 */
    double min_var;  /* MultivariateNormal.variance clamp; gpytorch min_variance = 1e-10 */
    int32_t params_const; /* 0 | 1.  1: the parameters are constants (acquisition optimisation against a fitted model) --
                           * honoured by mobocmf_layer_panel_* and mobocmf_panel_workspace_bytes, refused by the whole-call
                           * entry points */
    int32_t reserved;
    const mobocmf_tuning* tuning; /* kernel-selection knobs of THIS call and of the size queries made with this descriptor;
                                   * NULL = defaults */
    void* const* probe_events;    /* diagnostic, NULL = off: MOBOCMF_PROBE_EVENTS hipEvent_t (created by the caller with timing
                                   * enabled; NULL entries are skipped) recorded on the call's stream around the
                                   * grid-filling launches of this layer's PANEL half:
                                   *   [9] Gram forward [0] A = L^-1 K [1] C = U^T A [2]  ...  [3] dA [4] ... [5] weighted
                                   *   syrk + slab reduction [6] ... [7] dK = L^-T dA [8] Gram backward [10]
                                   * -- per-kernel durations inside a training step without a profiler (bench.py:
                                   * per_kernel_instep_ms).  Not under stream capture. */
} mobocmf_layer_desc;
#define MOBOCMF_PROBE_EVENTS 11

/* A layer call has two halves:
 *   CHAIN  the M x M work that depends on the parameters alone: K_mm, its Cholesky and inverse, U = L^-1 L_S,
 *          a = L^-1 m, the KL (forward); the M x M backward chain, Cholesky backward, Gram backward of K_mm (backward);
 *   PANEL  the M x N' work: K_mn, A, C, moments (forward); dA, the weighted syrk, dK, Gram backward of K_mn (backward).
 * mobocmf_layer_forward / _backward run both (desc->params_const must be 0); mobocmf_layers_chain_* and mobocmf_layer_panel_*
 * below run them apart, meeting in the layer's chain block. */

int mobocmf_version(void);
/* 1 if the current HIP device is gfx950. */
int mobocmf_device_arch_ok(void);

/* Bytes of the `saved` buffer (forward -> backward state: L, L^-1, U, K_mn, A, C, ...) and of the scratch
 * buffer (dead after each call). */
int mobocmf_layer_workspace_bytes(const mobocmf_layer_desc* desc, size_t* saved_bytes, size_t* scratch_bytes);

/* mean[Np], var[Np] (clamped at min_var), kl[1] = KL(q(u) || p(u)), info[1]. */
int mobocmf_layer_forward(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                          const double* zf, const double* hyp, const double* m, const double* L_S /* M x M, ld M */,
                          double* mean, double* var, double* kl, int32_t* info, void* saved, size_t saved_bytes,
                          void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);

/* Gradients of  sum(g_mean*mean) + sum(g_var*var) + g_kl[0]*kl.
 * Outputs (overwritten): g_f[Np] (kind 1), g_zf[M] (kind 1), g_hyp[hyp_len], g_m[M], g_LS[M x M] (lower),
 * g_x[(Np/xdiv) x d] (only if want_dx).  g_kl is a device scalar. */
int mobocmf_layer_backward(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                           const double* zf, const double* hyp, const double* m, const double* L_S,
                           const double* g_mean, const double* g_var, const double* g_kl, double* g_f, double* g_zf,
                           double* g_hyp, double* g_m, double* g_LS, double* g_x, void* saved, size_t saved_bytes,
                           void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);

/* ---- The same layer call for SEVERAL layers of one model (n <= 4, equal M): the CHAIN halves of all layers run as ONE
 * z-batched sequence of launches.  A chain is a serial string of latency-bound M x M kernels (Cholesky panels, triangular
 * inverse, a dozen M x M products); the layers' chains are independent of each other (Z~_l = [Z_x, m_{l-1}] depends on
 * parameters only), so batching them divides the length of that string by the number of layers.
 * Memory: one CHAIN BLOCK per layer (mobocmf_chain_block_bytes; all M x M-sized: the chain state L, L^-1, U, ... that the
 * PANEL halves read, H / Hc / da that the PANEL backward leaves for the chain backward, and the chain's scratch), the n
 * blocks `block_stride` bytes apart (a multiple of 256, >= the block size) starting at `blocks`, which holds `blocks_bytes`
 * >= n * block_stride bytes (checked: MOBOCMF_WORKSPACE_TOO_SMALL); per layer a PANEL `saved`
 * and `scratch` (mobocmf_panel_workspace_bytes).  Call order of a step: layers_chain_forward; layer_panel_forward per layer
 * (bottom up); layer_panel_backward per layer (top down); layers_chain_backward.  Arrays of pointers are HOST arrays of n
 * entries (device pointers inside).  The PANEL backward OVERWRITES g_hyp / g_zf with the K_mn share, the chain backward
 * OVERWRITES its own g_hyp / g_zf arguments with the K_mm share (the caller adds the two).  had_panel[l] = 0: layer l got no
 * upstream mean / var gradient (only its KL was differentiated); 1: its PANEL backward ran; 2: it ran AND the g_hyp[l] / g_zf[l]
 * passed to the chain backward already hold its share -- the chain backward adds to them instead of overwriting.
 * had_panel[l] |= 4 (l >= 1, kind 1): zf[l] IS the variational mean m[l-1] of the previous layer of this call (the reference's
 * Z~_l = [Z_x, m_{l-1}], mfdgp_hidden_layer.py:555-556): the complete gradient of zf[l] -- this call's K_mm share plus, under
 * 2, the PANEL share found in g_zf[l] -- is ADDED to g_m[l-1] and g_zf[l] is not written; the caller hands g_m[l-1] to m[l-1]
 * and nothing to zf[l].
 * The first `state_bytes` of a block (mobocmf_chain_block_bytes) are the CHAIN state the PANEL halves read; they do not depend
 * on Np.  desc->params_const = 1 (PANEL calls only): the parameters are constants.  `chain_block` may then be that state alone
 * (block_bytes >= state_bytes) and the call does not write through it -- a frozen state serves every evaluation of a search, on
 * any number of streams; the backward yields g_f / g_x (and the K_mn share of g_zf / g_hyp) and skips H / Hc / da, which only a
 * chain backward would consume. */
int mobocmf_chain_block_bytes(const mobocmf_layer_desc* desc, size_t* block_bytes, size_t* state_bytes);
int mobocmf_panel_workspace_bytes(const mobocmf_layer_desc* desc, size_t* saved_bytes, size_t* scratch_bytes);
int mobocmf_layers_chain_forward(int32_t n, const mobocmf_layer_desc* const* desc, const double* const* Zx,
                                 const double* const* zf, const double* const* hyp, const double* const* m,
                                 const double* const* L_S, double* const* kl, int32_t* const* info, void* blocks,
                                 size_t block_stride, size_t blocks_bytes, mobocmf_stream_t stream);
int mobocmf_layers_chain_backward(int32_t n, const mobocmf_layer_desc* const* desc, const double* const* Zx,
                                  const double* const* zf, const double* const* hyp, const double* const* g_kl,
                                  const int32_t* had_panel, double* const* g_zf, double* const* g_hyp, double* const* g_m,
                                  double* const* g_LS, void* blocks, size_t block_stride, size_t blocks_bytes,
                                  mobocmf_stream_t stream);
int mobocmf_layer_panel_forward(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                                const double* zf, const double* hyp, double* mean, double* var, void* chain_block,
                                size_t block_bytes, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                mobocmf_stream_t stream);
int mobocmf_layer_panel_backward(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                                 const double* zf, const double* hyp, const double* g_mean, const double* g_var,
                                 double* g_f, double* g_zf, double* g_hyp, double* g_x, void* chain_block,
                                 size_t block_bytes, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                 mobocmf_stream_t stream);

/* cov[Np x Np] = K_nn - A^T A + C^T C (A = L^-1 K_mn, C = U^T A): the full predictive covariance of the eval branch of the
 * variational strategy (the dense matrix GPyTorch materialises in .eval(), JESMOC_MFDGP.py:42 -> mfdgp.py:248), written as
 * the full symmetric matrix with leading dimension ldcov >= Np.  Only the layer's CHAIN state is read (`chain_state` = the
 * first `state_bytes` (mobocmf_chain_block_bytes) of the chain block mobocmf_layers_chain_forward filled: L^-1 and U), so a frozen
 * chain serves any number of input batches.  The contractions over the M inducing points are symmetric rank-M updates on
 * the MFMA (lower 128-tiles only), one column panel at a time: the scratch (mobocmf_predictive_covariance_workspace_bytes)
 * grows with Np x panel width, not Np^2, and Np is not capped.  Ordinary layer scratch sizes do not include it. */
int mobocmf_predictive_covariance_workspace_bytes(const mobocmf_layer_desc* desc, size_t* scratch_bytes);
int mobocmf_predictive_covariance(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                                  const double* zf, const double* hyp, double* cov, int64_t ldcov, const void* chain_state,
                                  size_t chain_state_bytes, void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);

/* Dense prior covariance K[i][j] = k([x1[i], f1[i]], [x2[j], f2[j]]) of one layer's kernel (the lazy prior of
 * MFDGPHiddenLayer.forward, mfdgp_hidden_layer.py:232-243, evaluated): x1 [n1 x d], x2 [n2 x d], f1 [n1] / f2 [n2] (kind 1,
 * else NULL).  K is row-major with ldk >= n2 and must hold round_up(n1, 32) rows (rows >= n1 are written as zeros). */
int mobocmf_gram_forward(int32_t kind, int32_t d, const double* x1, const double* f1, int64_t n1, const double* x2,
                         const double* f2, int64_t n2, const double* hyp, double* K, int64_t ldk, mobocmf_stream_t stream);
/* The same with the column side given as a layer gives it: nbase2 base rows x2 [nbase2 x d], each replicated xdiv times
 * (1..MOBOCMF_MAX_XDIV), column j = row j / xdiv of x2 with f2[j]; f2 holds nbase2 * xdiv values and K has nbase2 * xdiv
 * columns (ldk >= nbase2 * xdiv).  This is the launch of a layer's K_mn, replica fast paths included (xdiv 8 / 16 with f2
 * and K 16-byte aligned and ldk even; any other xdiv or alignment takes the general path, same values).  knn (may be NULL)
 * receives the nbase2 * xdiv prior variances k(column j, column j).  Columns >= nbase2 * xdiv of K are not written. */
int mobocmf_gram_forward_rep(int32_t kind, int32_t d, const double* x1, const double* f1, int64_t n1, const double* x2,
                             const double* f2, int64_t nbase2, int32_t xdiv, const double* hyp, double* K, int64_t ldk,
                             double* knn, mobocmf_stream_t stream);

/* The Gram backward of the same launch, alone: given G = dL/dK [n1 x nbase2 * xdiv] (row-major, ldk >= nbase2 * xdiv) and
 * gknn = dL/dknn (nbase2 * xdiv values, or NULL), the gradients of L with respect to hyp, f1, f2 and x2.  Arguments as in
 * mobocmf_gram_forward_rep: rows are x1 / f1, columns the rows of x2 replicated xdiv-fold with f2.  This is the launch that
 * ends a layer's PANEL backward (the Gram kernel writes per-workgroup partial sums, one reduction launch adds them up), the
 * replica fast paths included (kind 1, xdiv 8 / 16 with f2 and G 16-byte aligned and ldk even; anything else takes the
 * general path, same values up to summation order).
 *   G             rows >= n1 are never read.  col_activity (may be NULL = all active): one word per 128 columns,
 *                 ceil(nbase2 * xdiv / 128) words; the columns of a block whose word is zero are never read and count as exact
 *                 zeros (the block was never written, it may hold anything).
 *   gknn          is read at EVERY column, whatever col_activity says (a layer's is zero in inactive blocks).
 *   g_hyp         [1 + d] (kind 0) or [5 + 2 d] (kind 1), OVERWRITTEN, like every output.
 *   g_f1, g_f2    [n1], [nbase2 * xdiv]: kind 1 only (kind 0: not touched, may be NULL).  g_f2 is exactly 0 in an inactive
 *                 block when gknn is NULL or zero there.
 *   g_x2          [nbase2 x d], the gradient with respect to the column-side inputs; NULL = it is not formed.
 *   workspace     the partial sums, >= the bytes mobocmf_gram_backward_workspace_bytes reports for the same shape and
 *                 want_dx = (g_x2 != NULL); MOBOCMF_WORKSPACE_TOO_SMALL below that.  Nothing beyond the reported size is written.
 * geometry (may be NULL) receives the launch: [0] workgroups along the columns (128 base rows each), [1] along the rows,
 * [2] rows of x1 per workgroup (8, 16 or 32).  The partial counts the reduction sees follow from it: [0] * [1] for g_hyp,
 * [1] for g_f2 and g_x2, [0] for g_f1. */
int mobocmf_gram_backward_workspace_bytes(int32_t kind, int32_t d, int64_t n1, int64_t nbase2, int32_t xdiv, int32_t want_dx,
                                          size_t* bytes, int32_t* geometry);
int mobocmf_gram_backward(int32_t kind, int32_t d, const double* x1, const double* f1, int64_t n1, const double* x2,
                          const double* f2, int64_t nbase2, int32_t xdiv, const double* hyp, const double* G, int64_t ldk,
                          const double* gknn, const int32_t* col_activity, double* g_hyp, double* g_f1, double* g_f2,
                          double* g_x2, void* workspace, size_t workspace_bytes, mobocmf_stream_t stream);

/* The ROW-side input gradient of the same launch, the one output mobocmf_gram_backward does not form: g_x1 [n1 x d] =
 * dL/dx1 for L = sum G . K -- the gradient with respect to the inducing inputs Z_x when the rows are the inducing points.
 * Arguments as in mobocmf_gram_backward (rows x1 / f1, columns the rows of x2 replicated xdiv-fold with f2; G, ldk and
 * col_activity as there: rows >= n1 of G and the columns of inactive blocks are never read).  n1 <= 65535 * 64.
 *   symmetric     1 = the K_mm mode: n1 == nbase2, xdiv == 1 (MOBOCMF_BAD_ARG otherwise), x2 / f2 hold the values of x1 / f1
 *                 and G is symmetric; g_x1 is then the gradient with respect to the shared argument, row side plus column
 *                 side (twice the row side; the diagonal contributes nothing).  0 = the row side alone.
 *   g_x1          OVERWRITTEN.  Deterministic: per-chunk partial sums and one reduction launch, no atomics; two calls on
 *                 the same inputs give the same bits.
 *   workspace     >= the bytes mobocmf_gram_backward_rows_workspace_bytes reports; MOBOCMF_WORKSPACE_TOO_SMALL below that.
 *                 Nothing beyond the reported size is written.
 * geometry (may be NULL) receives the launch: [0] column chunks = partials per output the reduction adds, [1] row groups
 * (64 rows each), [2] base columns per chunk (four wavefronts, [2] / 4 base columns each, walked in tiles of 32 columns). */
int mobocmf_gram_backward_rows_workspace_bytes(int32_t kind, int32_t d, int64_t n1, int64_t nbase2, int32_t xdiv, size_t* bytes,
                                               int32_t* geometry);
int mobocmf_gram_backward_rows(int32_t kind, int32_t d, const double* x1, const double* f1, int64_t n1, const double* x2,
                               const double* f2, int64_t nbase2, int32_t xdiv, const double* hyp, const double* G, int64_t ldk,
                               const int32_t* col_activity, int32_t symmetric, double* g_x1, void* workspace,
                               size_t workspace_bytes, mobocmf_stream_t stream);

/* The backward halves with the gradient of the inducing inputs Z_x [M x d] as one more output.  Each takes the arguments of
 * the entry point it extends plus g_Zx and a workspace of its own (zws, zws_bytes), runs exactly that entry point's launches
 * -- every other output has the plain call's bits -- and then the row-side Gram backward on the dL/dK_mn (PANEL) or the
 * symmetrised dL/dK_mm (CHAIN) those launches left in the scratch / chain block.
 *   mobocmf_layer_backward_z          g_Zx = K_mn share + K_mm share, OVERWRITTEN; zws >= panel_bytes + chain_bytes.
 *   mobocmf_layer_panel_backward_z    g_Zx = the K_mn share, OVERWRITTEN; zws >= panel_bytes.  params_const = 1 is refused.
 *   mobocmf_layers_chain_backward_z   g_Zx = host array of n device pointers, each [M x d]: the K_mm shares, OVERWRITTEN;
 *                                     zws >= n * chain_bytes.
 * panel_bytes / chain_bytes: mobocmf_inducing_grad_workspace_bytes.  zws must not overlap the call's saved / scratch bytes or
 * chain blocks (MOBOCMF_BAD_ARG).  For layers >= 1 the gradient holds for a Z_x shared by all layers of the model (Z~_l =
 * [Z_x, m_{l-1}]): the caller adds the layers' shares. */
int mobocmf_inducing_grad_workspace_bytes(const mobocmf_layer_desc* desc, size_t* panel_bytes, size_t* chain_bytes);
int mobocmf_layer_backward_z(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                             const double* zf, const double* hyp, const double* m, const double* L_S,
                             const double* g_mean, const double* g_var, const double* g_kl, double* g_f, double* g_zf,
                             double* g_hyp, double* g_m, double* g_LS, double* g_x, double* g_Zx, void* saved,
                             size_t saved_bytes, void* scratch, size_t scratch_bytes, void* zws, size_t zws_bytes,
                             mobocmf_stream_t stream);
int mobocmf_layer_panel_backward_z(const mobocmf_layer_desc* desc, const double* x, const double* f, const double* Zx,
                                   const double* zf, const double* hyp, const double* g_mean, const double* g_var,
                                   double* g_f, double* g_zf, double* g_hyp, double* g_x, double* g_Zx, void* chain_block,
                                   size_t block_bytes, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                   void* zws, size_t zws_bytes, mobocmf_stream_t stream);
int mobocmf_layers_chain_backward_z(int32_t n, const mobocmf_layer_desc* const* desc, const double* const* Zx,
                                    const double* const* zf, const double* const* hyp, const double* const* g_kl,
                                    const int32_t* had_panel, double* const* g_zf, double* const* g_hyp, double* const* g_m,
                                    double* const* g_LS, double* const* g_Zx, void* blocks, size_t block_stride,
                                    size_t blocks_bytes, void* zws, size_t zws_bytes, mobocmf_stream_t stream);

/* One random-Fourier-feature function sample of a layer evaluated at n points (mfdgp_hidden_layer.py:326-337, :402-444; the
 * Pareto-grid evaluation of moop.py:232-272), without materialising the F x n feature matrix:
 *   kind 0:  out[i] = sum_j theta[j] s0 cos(W1[j].x_i + b1[j])
 *   kind 1:  out[i] = sum_j theta[j] s0 fprev[i] cos(W1[j].x_i + b1[j]) + theta[F+j] s1 cos(W1[j].x_i + Wf[j] fprev[i] + b1[j])
 *                          + theta[2F+j] s2 cos(W2[j].x_i + b2[j])
 * x [n x d], W1 / W2 [F x d], b1 / b2 / Wf [F], theta [F] or [3F]; fprev = the previous layer's sample at the same points
 * (the layer recursion is one call per layer).  s0 = sqrt(2 alpha / F) (kind 0) resp. sqrt(2 a1 nu / F), s1 = sqrt(2 a1 af / F),
 * s2 = sqrt(2 a2 / F). */
int mobocmf_rff_eval(int32_t kind, int32_t d, int32_t F, int64_t n, const double* x, const double* fprev, const double* W1,
                     const double* b1, const double* Wf, const double* W2, const double* b2, const double* theta, double s0,
                     double s1, double s2, double* out, mobocmf_stream_t stream);

/* K chain samples (a layer-0 sample and the layers >= 1 recursing on it, the whole function sample of one black-box) at the
 * same n points in ONE launch: out[k * n + i] = the top layer of sample k at x_i.  The layer recursion stays in a register,
 * nothing goes back to memory between layers.  params: the samples' operands, ONE device buffer of doubles; desc: DEVICE table
 * of K * MOBOCMF_RFF_MAX_LAYERS entries, entry k * MOBOCMF_RFF_MAX_LAYERS + l = layer l of sample k (kind 0 for l = 0, kind 1
 * above it, kind -1 after the top layer; the formulas, operand shapes and scales of mobocmf_rff_eval, operands at the given
 * offsets into params).  A layer whose operands do not lie inside params_len doubles writes NaN for its sample.  Deterministic
 * (no atomics): two launches give bitwise identical output. */
#define MOBOCMF_RFF_MAX_LAYERS 3
typedef struct mobocmf_rff_layer_desc {
    int32_t kind;                       /* 0, 1, or -1 = no such layer */
    int32_t F;                          /* features */
    int64_t W1, b1, theta, Wf, W2, b2;  /* offsets (doubles) into params: W1 / W2 [F x d], b1 / b2 / Wf [F], theta [F] or [3F] */
    double s0, s1, s2;                  /* the scales of mobocmf_rff_eval */
} mobocmf_rff_layer_desc;
int mobocmf_rff_eval_chains(int32_t K, int32_t d, int64_t n, const double* x, const double* params, int64_t params_len,
                            const mobocmf_rff_layer_desc* desc, double* out, mobocmf_stream_t stream);

/* K chain samples AND their input gradients at n points: vals[k * n + i] = sample k at x_i (the value of
 * mobocmf_rff_eval_chains, another summation order), grads[(k * n + i) * d + c] = d sample_k / d x_c at x_i.  Operands: those of
 * mobocmf_rff_eval_chains.  Forward mode through the layer recursion, df_l/dx = (partial f_l / partial x) +
 * (partial f_l / partial f_{l-1}) df_{l-1}/dx, with per feature j of kind 1
 *   d/dx     = -(theta[j] s0 fprev sin(a1) + theta[F+j] s1 sin(a1 + Wf[j] fprev)) W1[j] - theta[2F+j] s2 sin(a2) W2[j]
 *   d/dfprev =   theta[j] s0 cos(a1) - theta[F+j] s1 Wf[j] sin(a1 + Wf[j] fprev)           (a1 = W1[j].x + b1[j], a2 likewise)
 * One wavefront per (sample, point): the features are split over its 64 lanes and summed across them in a fixed order.  A
 * layer whose operands do not lie inside params_len doubles writes NaN for its sample (values and gradients) and is never
 * read.  Deterministic (no atomics): two launches give bitwise identical output. */
int mobocmf_rff_chains_value_grad(int32_t K, int32_t d, int64_t n, const double* x, const double* params, int64_t params_len,
                                  const mobocmf_rff_layer_desc* desc, double* vals, double* grads, mobocmf_stream_t stream);

/* Settings of mobocmf_rff_refine; they travel with the call (NULL = the defaults mobocmf_rff_refine_options_init writes). */
typedef struct mobocmf_rff_refine_options {
    uint32_t struct_size;   /* sizeof(mobocmf_rff_refine_options) of the caller (set by mobocmf_rff_refine_options_init) */
    int32_t outer;          /* multiplier rounds (default 8, 1..64) */
    int32_t inner;          /* projected-gradient steps per round (default 30, 1..1024) */
    int32_t backtracks;     /* step reductions per inner step after its first trial (default 6, 0..32) */
    int32_t restore;        /* feasibility-restoration steps after the last round (default 4, 0..32) */
    int32_t recentre;       /* 1 (default): after a round that did not cut the largest violation to a quarter, the next round
                             * starts from the start's best feasible point so far (the iterate may have strayed into another
                             * basin of a nonconvex constraint); 0: it continues from the iterate */
    double step0;           /* initial step (default 0.05) */
    double step_shrink;     /* factor of one backtrack (default 0.25, in (0, 1)) */
    double step_grow;       /* factor on an accepted step when the curvature estimate is unusable (default 2, >= 1) */
    double rho0;            /* initial penalty (default 10) */
    double rho_growth;      /* penalty factor when the largest violation did not fall to a quarter (default 4, >= 1) */
    double armijo;          /* sufficient-decrease constant (default 1e-4, in (0, 1)) */
    double restore_margin;  /* slack the restoration aims for (default 1e-9, >= 0) */
} mobocmf_rff_refine_options;
int mobocmf_rff_refine_options_init(mobocmf_rff_refine_options* opt);

/* Constrained multi-start refinement of chain samples in one launch (the refinement stage of MOOP): problem p minimises chain
 * obj[p] over the box [0, 1]^d subject to chain(con[con_off[p] + i])(x) - thr[con_off[p] + i] >= 0, i < con_cnt[p], from the R
 * starts x0[p][r].  params / params_len / desc: the K chains, as for mobocmf_rff_eval_chains.  obj, con_off, con_cnt [P] are
 * HOST arrays (they travel as launch arguments; P <= MOBOCMF_REFINE_MAX_PROBLEMS, con_cnt[p] <= MOBOCMF_REFINE_MAX_CON);
 * con [n_con] (int32) and thr [n_con] are DEVICE arrays (NULL when n_con = 0).
 *
 * Method, per start, on one workgroup (features over its lanes, sums in a fixed order): augmented Lagrangian in the
 * Powell-Hestenes-Rockafellar form, merit = f + sum_i (max(0, lambda_i - rho s_i)^2 - lambda_i^2) / (2 rho) with the slacks
 * s_i; `inner` projected-gradient steps per round, each with Armijo backtracking on the merit (first trial step: the
 * Barzilai-Borwein estimate of the last accepted step, else step_grow times it); after a round lambda_i = max(0, lambda_i -
 * rho s_i) and rho grows when the largest violation did not fall to a quarter (the next round then restarts from the best
 * feasible point found so far, see `recentre`); after the last round up to `restore` steps
 * x <- clamp(x - (2 V / |grad V|^2) grad V), V = 1/2 sum_i max(0, restore_margin - s_i)^2, bring an iterate that ends just
 * outside the feasible set back into it.  Every trip count is fixed by the options: no data-dependent waits, no workgroup
 * waits on another.  Every iterate is clamped to the box.
 *
 * Per start:   xs [P x R x d], fs [P x R], slack_min [P x R] = the best FEASIBLE point evaluated (by the kernel's own values:
 *              every slack >= 0), the start (clamped) included -- so fs <= f(x0) for a feasible start -- its value and its
 *              smallest slack (+inf without constraints).  No feasible point (or a NaN start, which is not iterated): fs =
 *              NaN, xs / slack_min = the last iterate (the start itself if it held a NaN).
 * Per problem: x_best [P x d], f_best [P], start_best [P] (int32) = the start result with the smallest fs, ties to the lowest r
 *              (reduced on the device by a second small launch on the same stream); status [P] (int32): 0 = refinement moved
 *              away from that start, 1 = x_best is the (clamped) start start_best itself, 2 = no start has a feasible result
 *              (an invalid descriptor or chain index, NaN or infeasible starts): f_best = NaN, start_best = -1, x_best = NaN.
 * Bitwise reproducible across launches.  MOBOCMF_BAD_ARG: a null pointer, P < 1, P > MOBOCMF_REFINE_MAX_PROBLEMS, R < 1, d
 * outside 1..MOBOCMF_MAX_D, K < 1, obj[p] outside [0, K), con_cnt[p] < 0 or > MOBOCMF_REFINE_MAX_CON, a constraint range
 * outside [0, n_con), or options outside their ranges. */
#define MOBOCMF_REFINE_MAX_PROBLEMS 64
#define MOBOCMF_REFINE_MAX_CON 32
int mobocmf_rff_refine(int32_t P, int32_t R, int32_t d, int32_t K, const int32_t* obj, const int32_t* con_off,
                       const int32_t* con_cnt, int32_t n_con, const int32_t* con, const double* thr, const double* x0,
                       const double* params, int64_t params_len, const mobocmf_rff_layer_desc* desc,
                       const mobocmf_rff_refine_options* opt, double* xs, double* fs, double* slack_min, double* x_best,
                       double* f_best, int32_t* start_best, int32_t* status, mobocmf_stream_t stream);

/* Feasibility of grid rows under K_con sampled constraints (MOOP.find_feasible_grid): vals [K_con x n] with row stride ldv
 * (>= n), thr [K_con]; slack = vals[c][i] - thr[c].  ok[i] = 1 if every slack >= 0 else 0; viol[i] = sum_c min(slack, 0)
 * summed in the order c = 0, 1, ... */
int mobocmf_rff_feasibility(int32_t K_con, int64_t n, const double* vals, int64_t ldv, const double* thr, int32_t* ok,
                            double* viol, mobocmf_stream_t stream);

/* Recommendation of the BO driver: the probably-feasible, non-dominated rows of predicted objectives (all minimised).
 * vals [k x n] with row stride ldv (>= n); con_mean / con_var [K_con x n] with row stride ldc (>= n), the Gaussian predictions
 * of K_con constraints (K_con = 0: every row is feasible, the pointers may be NULL); noise [K_con] subtracted from the
 * variances (NULL = none).  Row i is feasible when 0.5 erfc(-(m / sqrt(v - noise)) / sqrt(2)) > p_min for every constraint:
 * v - noise < 0 makes it infeasible, v - noise == 0 leaves the sign of m to decide.  mask[i] = 1 for the rows of the front:
 * feasible, no NaN objective, and no other such row j with vals[.][j] <= vals[.][i] everywhere and either != somewhere or
 * j < i (MOOP.compute_pareto_front on the feasible rows: of exactly equal rows the first is kept); 0 otherwise.
 * counts [3] (DEVICE): feasible rows, front rows, feasible rows with a NaN objective (they are never kept and dominate
 * nothing).  1 <= k <= MOBOCMF_PARETO_MAX_K, 0 <= n <= 2^31 - 1.  Deterministic; three launches on `stream`, no workspace. */
#define MOBOCMF_PARETO_MAX_K 16
int mobocmf_pareto_mask(int32_t k, int64_t n, const double* vals, int64_t ldv, int32_t K_con, const double* con_mean,
                        const double* con_var, int64_t ldc, const double* noise, double p_min, int32_t* mask, int64_t* counts,
                        mobocmf_stream_t stream);

/* Exact hypervolume of P points [P x k] (row stride ldp >= k, all objectives minimised) against ref [k] (DEVICE): the volume of
 * the union of the boxes [p, ref] over the points that weakly dominate ref (the others add nothing, pymoo's rule); duplicates
 * and dominated points are allowed, P = 0 gives 0.  Work O(P^(k-1)): 1 <= k <= MOBOCMF_HV_MAX_K and P <= 65536 (k <= 3),
 * 1024 (k = 4), 256 (k = 5), MOBOCMF_BAD_ARG beyond.  Host-side, synchronising: *hv is a HOST double, written after the
 * launches on `stream` have finished; NaN in the points or in ref returns MOBOCMF_BAD_ARG.  Bitwise reproducible (fixed
 * summation order, no floating-point atomics).  workspace: mobocmf_hypervolume_workspace_bytes(k, P) bytes of device memory. */
#define MOBOCMF_HV_MAX_K 5
int mobocmf_hypervolume_workspace_bytes(int32_t k, int64_t P, size_t* bytes);
int mobocmf_hypervolume(int32_t k, int64_t P, const double* pts, int64_t ldp, const double* ref, double* hv, void* workspace,
                        size_t workspace_bytes, mobocmf_stream_t stream);

/* ------------------------------------------------------------------ NSGA-II over chain samples (csrc/pareto_evolve.hip)
 * The population logic of an elitist non-dominated-sorting search (Deb et al. 2002) on rows of the box [0, 1]^d whose k
 * objectives (all minimised) and violation were computed elsewhere (mobocmf_rff_eval_chains / mobocmf_rff_feasibility).
 * Everything is float64, deterministic and bitwise reproducible across launches: no floating-point atomics, no workgroup
 * waits on another, every trip count is bounded by the row count.
 *
 * mobocmf_nsga_survive ranks n_in rows and keeps n_keep of them.
 *   Inputs.  X [n_in x d] row-major; F [k x n_in], objective j of row i at F[j * ldf + i] (ldf >= n_in); viol [n_in], the
 *   violation: >= 0, 0 = feasible (the caller passes MINUS the viol of mobocmf_rff_feasibility; -0.0 is 0); NULL = every row
 *   is feasible.  A row with a NaN objective or a NaN violation is infeasible with violation +inf.
 *   Constraint-domination.  Row i dominates row j when (a) i is feasible and j is not, or (b) both are infeasible and
 *   viol_i < viol_j, or (c) both are feasible, F[c][i] <= F[c][j] for every c and F[c][i] < F[c][j] for some c.  Exactly equal
 *   rows do not dominate each other.
 *   Rank = peeling depth: rank 0 holds the rows nobody dominates; remove them and repeat for rank 1, ...
 *   Crowding, per rank, starts at 0 and takes one term per objective c = 0, 1, ..., k - 1 in that order.  A NaN objective value
 *   counts as +inf here.  Order the rank's rows by (value, row index); prev / next = the neighbours of a row in that order,
 *   min / max = the first / last value.  The first and the last row add +inf; an interior row adds
 *   (next - prev) / (max - min) -- one IEEE subtraction each, one division, then one addition to the running sum -- and adds 0
 *   when max == min or when the quotient is NaN (inf - inf, inf / inf).
 *   Survivors = the first n_keep rows under the key (rank ascending, crowding descending, row index ascending); equal
 *   crowding (+inf == +inf included) falls through to the index.
 *   Outputs, compacted in key order: X_out [n_keep x d], F_out [k x n_keep] with row stride ldf_out (>= n_keep), viol_out
 *   [n_keep] (the violation as used: +inf for a NaN row; may be NULL when viol is NULL, else zeros are written), rank_out
 *   (int32), crowd_out, src_out (int32: the input row a survivor came from).  X_out / F_out / viol_out may BE the inputs (same
 *   base pointer, ldf_out == ldf): every survivor is read before any is written; any other overlap is not allowed.
 *   generation: NULL, or a DEVICE int64 word that this launch increments by one after everything else (what
 *   mobocmf_nsga_vary reads: a captured generation replays with a fresh generation number without the host).
 *   n_keep == n_in is the "rank only" call.  One launch of one workgroup: the n_in x n_in dominance relation is a bit matrix
 *   in LDS (128 KB at n_in = 1024), peeled with workgroup barriers; order positions and crowding neighbours by counting.
 *   MOBOCMF_BAD_ARG (before any launch): k outside 1..MOBOCMF_PARETO_MAX_K, d outside 1..MOBOCMF_MAX_D, not
 *   2 <= n_keep <= n_in <= MOBOCMF_NSGA_MAX_ROWS, ldf < n_in, ldf_out < n_keep, a NULL X, F, X_out, F_out, rank_out, crowd_out
 *   or src_out, viol given without viol_out.
 *
 * mobocmf_nsga_vary makes Np children (Np even, 2 <= Np <= MOBOCMF_NSGA_MAX_ROWS) from Np ranked parents X [Np x d] with rank /
 * crowd [Np] (what mobocmf_nsga_survive wrote).  Every uniform is u(s) = philox_uniform(seed, *generation, q * 2^32 + s): the
 * Philox4x32-10 stream keyed by seed, counter (q * 2^32 + s, *generation), 53 bits -> (0, 1), of mobocmf_propagate_rng_forward;
 * q = the pair, s = the slot below; *generation is the DEVICE int64 word.  Pair q < Np / 2 gives children 2 q and 2 q + 1.
 *   Tournament.  Parent e (0, 1) is the better of rows a = min(floor(u(2 e) Np), Np - 1) and b = min(floor(u(2 e + 1) Np),
 *   Np - 1): a wins when rank_a < rank_b, or the ranks are equal and (crowd_a > crowd_b, or crowd_b is not > crowd_a and
 *   a <= b); else b.
 *   Crossover (simulated binary).  The pair crosses when u(4) < p_c; then variable v crosses when u(8 + 8 v) < 0.5, with
 *   w = u(9 + 8 v), beta = (2 w)^(1 / (eta_c + 1)) for w <= 0.5 else (1 / (2 (1 - w)))^(1 / (eta_c + 1)),
 *   c0 = 0.5 ((1 + beta) p0 + (1 - beta) p1), c1 = 0.5 ((1 - beta) p0 + (1 + beta) p1).  Otherwise c0 = p0, c1 = p1.
 *   Mutation (polynomial).  Variable v of child e mutates when u(10 + 8 v + 2 e) < p_m; with w = u(11 + 8 v + 2 e),
 *   x += (2 w)^(1 / (eta_m + 1)) - 1 for w < 0.5 else x += 1 - (2 (1 - w))^(1 / (eta_m + 1)).
 *   Then x = min(max(x, 0), 1).
 *   Arithmetic.  Every operation above is one IEEE float64 operation as written, left to right, nothing fused, and a power
 *   x^e (x > 0) is NOT the math library's: it is pw(x, e) = ex(e * lg(x)), made of IEEE operations only, so that two
 *   implementations of this text agree in every bit (a child of two equal parents equals them or differs in the last place
 *   depending on the last bit of beta, and which of the two it is decides a domination).  With L = 0.6931471805599453:
 *     lg(x): x = m 2^n with 0.5 <= m < 1 (frexp); if m < 0.7071067811865476 then m = 2 m, n = n - 1; s = (m - 1) / (m + 1),
 *            z = s s; P = 1 / 23; for j = 21, 19, ..., 1: P = P z + 1 / j; lg = n L + (2 s) P.
 *     ex(y): n = rint(y * 1.4426950408889634) (to nearest, ties to even); r = y - n L; T = 1; for j = 14, 13, ..., 1:
 *            T = 1 + (r T) / j; ex = T 2^n (ldexp).
 *   children [Np x d] must not overlap X.  parents (NULL or int32 [Np]): parents[2 q + e] = the
 *   tournament winner e of pair q.
 *   MOBOCMF_BAD_ARG (before any launch): Np odd or outside its range, d outside 1..MOBOCMF_MAX_D, a NULL X, rank, crowd,
 *   generation or children, options of another struct_size or outside their ranges. */
#define MOBOCMF_NSGA_MAX_ROWS 1024
typedef struct mobocmf_nsga_options {
    uint32_t struct_size;   /* sizeof(mobocmf_nsga_options) of the caller (set by mobocmf_nsga_options_init) */
    uint32_t reserved;      /* 0 */
    double eta_c;           /* crossover distribution index (default 15, 0..1000) */
    double p_c;             /* crossover probability per pair (default 0.9, 0..1) */
    double eta_m;           /* mutation distribution index (default 20, 0..1000) */
    double p_m;             /* mutation probability per child and variable (default 0 = 1 / d, 0..1) */
} mobocmf_nsga_options;
int mobocmf_nsga_options_init(mobocmf_nsga_options* opt);
int mobocmf_nsga_survive(int32_t n_in, int32_t n_keep, int32_t d, int32_t k, const double* X, const double* F, int64_t ldf,
                         const double* viol, double* X_out, double* F_out, int64_t ldf_out, double* viol_out,
                         int32_t* rank_out, double* crowd_out, int32_t* src_out, int64_t* generation,
                         mobocmf_stream_t stream);
int mobocmf_nsga_vary(int32_t Np, int32_t d, const double* X, const int32_t* rank, const double* crowd, uint64_t seed,
                      const int64_t* generation, const mobocmf_nsga_options* opt, double* children, int32_t* parents,
                      mobocmf_stream_t stream);

/* ------------------------------------------------------------------ the recommendation's NSGA operands (csrc/recommend.hip)
 * What mobocmf_nsga_survive ranks when the rows are scored by fitted surrogates instead of chain samples (BlackBoxMFDGPFitter.
 * recommend(search="evolve")): the objectives are the surrogates' top-fidelity predictive means, the violation grades the
 * feasibility rule of mobocmf_pareto_mask.  It turns a predict group's raw top-layer moments into F and viol in ONE launch on
 * `stream`; no atomics, a fixed summation order (two calls on the same inputs are bitwise equal); it allocates nothing, reads
 * nothing on the host and keeps no state: capturable.
 *   moments  (n_obj + n_con, 2, T S): per model its means, then its variances WITHOUT noise, column t S + s (the moments of a
 *            predict group); the n_obj objectives come first, then the n_con constraints.
 *   scale    NULL, or (n_obj + n_con, 2): (shift, factor) per model -- recommend's output_scaling (mean, std).
 * Per model and test point t -- every operation below is one IEEE float64 operation as written, nothing fused:
 *   S = 1:  mbar = mu_0, v = var_0 exactly.
 *   else:   a = 0, q = 0; for s = 0 .. S - 1 in order: a = a + mu_s, q = q + (var_s + mu_s * mu_s);
 *           mbar = a / S, v = q / S - mbar * mbar.
 *   scale:  mbar = mbar * factor + shift, v = (v * factor) * factor.
 * Objective j (minimised): F[j * ldf + t] = mbar_j (ldf >= T).
 * Constraint c: z = mbar / sqrt(v).  It is feasible iff 0.5 erfc(-(z / sqrt(2))) > p_min -- the rule of mobocmf_pareto_mask on
 *   noise-free variances: v < 0 is infeasible, at v == 0 the sign of mbar decides.  viol_c = 0 when feasible, else
 *   max(z_min - z, DBL_MIN); viol_c = +inf when v < 0 or z is NaN.  viol[t] = sum_c viol_c, summed from 0.0 in the order of c
 *   (n_con = 0: 0.0, and viol may be NULL).
 *   z_min: the caller passes Phi^-1(p_min).  It only GRADES infeasible rows -- a violation measured in probability is flat where
 *   Phi saturates, and a constraint-domination search among infeasible rows needs a slope -- and never decides feasibility:
 *   viol[t] == 0 exactly where every constraint passes the rule above.
 * sqrt and the division of z are the only operations the stated order does not pin to the bit.
 * One launch of T workgroups of one wavefront: a lane per model sums its S samples in order, one lane adds the constraints'
 * terms in order.
 * MOBOCMF_BAD_ARG (on the host, before any HIP call): moments or F NULL; n_obj outside 1..MOBOCMF_PARETO_MAX_K; n_con < 0;
 * n_obj + n_con > 64; T < 1; S < 1; T S > MOBOCMF_ACQ_MAX_COLUMNS; ldf < T; viol NULL with n_con > 0; p_min not inside (0, 1);
 * z_min not finite. */
int mobocmf_recommend_scores(const double* moments, int32_t n_obj, int32_t n_con, int32_t T, int32_t S, const double* scale,
                             double p_min, double z_min, double* F, int64_t ldf, double* viol, mobocmf_stream_t stream);

/* Inducing-point selection by greedy conditional variance: the incomplete pivoted Cholesky of K_nn under the kind-0 kernel
 * (the one mobocmf_gram_forward(kind 0) evaluates).  x [N x d] row-major (1 <= d <= MOBOCMF_MAX_D), hyp = [a, ls[0..d)].
 * Step j picks the row with the largest residual d = diag(K_nn - K_nm K_mm^-1 K_mn) over the rows picked so far -- of
 * bitwise-equal residuals the lowest row, so step 0 is row 0 -- and stops before a pick whose residual is <= tol_rel * a or
 * not positive (tol_rel = 0: until max_points).  Residuals are clamped at 0 after every update; a picked row's is exactly 0.
 * Outputs (all DEVICE): idx [max_points] rows in pick order (-1 beyond count), count [1], resid [max_points] the residual of
 * each pick when it was picked (0 beyond count), diag [N] the final residuals, info [1].
 * Refusals.  MOBOCMF_BAD_ARG (host-visible, nothing is launched): N < 1, N > MOBOCMF_INDUCING_MAX_ROWS, max_points < 1,
 * > N or > MOBOCMF_INDUCING_MAX_POINTS, d out of range, tol_rel negative or not finite, form not 0 / 1 / 2, form 1 with
 * N > MOBOCMF_INDUCING_ONE_WG_MAX_ROWS (one compute unit would be held for minutes), a NULL pointer, a
 * workspace smaller than mobocmf_select_inducing_workspace_bytes(N, max_points).  info (device-visible): 1 = a non-finite
 * entry of x, 2 = a hyper-parameter that is non-finite, not positive, or a lengthscale whose reciprocal overflows; then
 * count = 0, idx = -1, resid and diag NaN.  info = 0 otherwise.  No host synchronisation inside the call.
 * form: 0 = by size | 1 = one workgroup, one launch, all steps (the BO loop's sizes) | 2 = one launch per pivot over many
 * workgroups (max_points + 3 launches; the pivot stays on the device, launches after the stop do nothing).  A row's
 * update is the same instruction sequence in one thread in both forms: idx, resid and diag are bitwise equal between them
 * and from run to run.
 * workspace: 32 KiB + N * max_points doubles of device memory (the factor, [max_points][N]): 32 MiB at N = 8192,
 * max_points = 512 (resident in the Infinity Cache), 512 MiB at N = 65536, max_points = 1024. */
#define MOBOCMF_INDUCING_MAX_POINTS 4096
#define MOBOCMF_INDUCING_MAX_ROWS 262144
#define MOBOCMF_INDUCING_ONE_WG_MAX_ROWS 32768
int mobocmf_select_inducing_workspace_bytes(int64_t N, int32_t max_points, size_t* bytes);
int mobocmf_select_inducing(int64_t N, int32_t d, const double* x, const double* hyp, int32_t max_points, double tol_rel,
                            int32_t form, int32_t* idx, int32_t* count, double* resid, double* diag, int32_t* info,
                            void* workspace, size_t workspace_bytes, mobocmf_stream_t stream);

/* ---- Mini-batches drawn on the device.  Replaces the host loader -- DataLoader(dataset, batch_size, shuffle=True),
 * blackbox_mfdgp_fitter.py:35 -- and the batch loop of the epoch closure (:156-173) inside a captured step: a replay sees a fresh
 * batch without the host.  Epoch e visits the rows in the order of a stateless keyed bijection of 0..N-1 (a Feistel network
 * with Philox4x32-10 round functions keyed by (seed, e, round), cycle-walking for values >= N; csrc/minibatch_perm.h, DESIGN
 * 5.3): position i of epoch e is a pure function of (seed, e, N, i).  Batch k of an epoch holds positions kB .. min((k+1)B, N)-1;
 * there are nb = ceil(N / B) batches, the last one ragged when B does not divide N (the loader's drop_last = False).
 *
 * state: 3 DEVICE int64 {seed, step, status}, caller-owned; step counts the batches drawn so far (epoch = step / nb,
 *   k = step % nb), status is 0 or a sticky MOBOCMF_MINIBATCH_* code.
 * mobocmf_minibatch_indices (one workgroup): writes src[0..rows) = the source rows of the batch (int64), with order_by_fidelity = 1
 *   sorted stably by DESCENDING fidelity (fid[row] truncated to an integer level, clamped to 0..L-1) so that the rows no upper
 *   layer needs are contiguous at the end; writes counts[l] = #{rows of the batch with fid >= l}, l < L (int64); advances step.
 *   Guard: rows_expected is the number of rows the caller's buffers (and its captured graph) are made for.  If batch k has a
 *   different number, or step is negative, or status is already set, the launch sets status and writes neither src, counts nor
 *   step; it never writes beyond rows_expected entries of src.
 * mobocmf_minibatch_gather (grid-wide, whole rows): xb[r][:] = x[src[r]][:], yb[r] = y[src[r]], fidb[r] = fid[src[r]] for
 *   r < rows, x [N x d] row-major; 16-byte accesses when d is even and x / xb are 16-byte aligned.  Rows whose src is outside
 *   0..N-1 are skipped; nothing is written when status is set.
 * mobocmf_minibatch_accumulate: sums[0..1] += (loss, kl) of the step just taken (restarted at the first batch of an epoch),
 *   sums[2..3] = the sums of the last finished epoch -- what the reference prints per epoch (:156-173) -- without a host read.
 * mobocmf_minibatch_permutation_host: out[i] = source row of position i of the epoch, on the HOST, from the same definition:
 *   for tests and for callers that ask which rows a step used.  Not a training path.
 * MOBOCMF_BAD_ARG (host-visible, nothing is launched): N < 1 or > MOBOCMF_MINIBATCH_MAX_ROWS, B < 1 or >= that bound, L < 1 or
 *   > MOBOCMF_MINIBATCH_MAX_LEVELS, d < 1 or > MOBOCMF_MAX_D, rows_expected < 1 or > min(B, N), rows > N, a negative epoch, a NULL
 *   pointer. */
#define MOBOCMF_MINIBATCH_MAX_ROWS 2147483648LL
#define MOBOCMF_MINIBATCH_MAX_LEVELS 8
#define MOBOCMF_MINIBATCH_ROWS_MISMATCH 1
#define MOBOCMF_MINIBATCH_BAD_STATE 2
int mobocmf_minibatch_permutation_host(int64_t seed, int64_t epoch, int64_t N, int64_t* out);
int mobocmf_minibatch_indices(int64_t N, int64_t B, int32_t L, const double* fid, int32_t order_by_fidelity,
                              int64_t rows_expected, int64_t* state, int64_t* src, int64_t* counts, mobocmf_stream_t stream);
int mobocmf_minibatch_gather(int64_t N, int32_t d, int64_t rows, const double* x, const double* y, const double* fid,
                             const int64_t* src, const int64_t* state, double* xb, double* yb, double* fidb,
                             mobocmf_stream_t stream);
int mobocmf_minibatch_accumulate(int64_t N, int64_t B, const int64_t* state, const double* loss, const double* kl, double* sums,
                                 mobocmf_stream_t stream);

/* f~[n] = mean[n/div] + sqrt(var[n/div]) * eps[n],  n < n_out  (mfdgp_hidden_layer.py:263-274). */
int mobocmf_propagate_forward(const double* mean, const double* var, const double* eps, double* f_out, int64_t n_out,
                              int32_t div, mobocmf_stream_t stream);
/* The same with eps ~ N(0, 1) drawn inside the launch (the reference draws it with torch.normal, mfdgp_hidden_layer.py:274):
 * counter-based Philox4x32-10 keyed by (seed, call counter, row index), Box-Muller in float64.  rng_state = 3 device int64
 * {seed, calls, ticket} owned by the caller (ticket zero before the first call; every call leaves it zero and advances
 * `calls` by one, so a captured step replays with fresh eps).  eps_out[n_out] receives the draw (the backward pass needs it). */
int mobocmf_propagate_rng_forward(const double* mean, const double* var, int64_t* rng_state, double* f_out, double* eps_out,
                                  int64_t n_out, int32_t div, mobocmf_stream_t stream);
/* g_mean[n_out/div], g_var[n_out/div] from g_f[n_out]. */
int mobocmf_propagate_backward(const double* var, const double* eps, const double* g_f, double* g_mean, double* g_var,
                               int64_t n_out, int32_t div, mobocmf_stream_t stream);
/* Prefix propagation: the previous layer holds n_prev >= n_out/div rows of which only the FIRST n_out/div were propagated
 * (the next layer is evaluated on a prefix of the batch -- the rows that can reach the loss, see mobocmf_elbo_forward);
 * g_mean / g_var [n_prev] get zeros beyond the prefix.  add_mean / add_var [n_prev] (each may be NULL): gradients the same
 * moments receive from their other consumer -- the ELBO data term of the previous layer's own fidelity
 * (variational_elbo_mf.py:33-35) -- added in this launch (autograd would spend one element-wise launch per sum). */
int mobocmf_propagate_backward_prefix(const double* var, const double* eps, const double* g_f, double* g_mean, double* g_var,
                                      int64_t n_out, int32_t div, int64_t n_prev, const double* add_mean,
                                      const double* add_var, mobocmf_stream_t stream);

/* out[0] = (1/div) * sum_{n : fid[n/div] == level} -0.5 * (((y[n/div]-mean[n])^2 + var[n]) / tau + log tau + log 2pi)
 * tau is a device scalar.  n < n_rows. */
int mobocmf_elbo_data_forward(const double* mean, const double* var, const double* y, const double* fid,
                              const double* tau, double level, int64_t n_rows, int32_t div, double* out,
                              void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);
/* g_mean[n_rows], g_var[n_rows], g_tau[1] scaled by the device scalar g_out. */
int mobocmf_elbo_data_backward(const double* mean, const double* var, const double* y, const double* fid,
                               const double* tau, double level, int64_t n_rows, int32_t div, const double* g_out,
                               double* g_mean, double* g_var, double* g_tau, void* scratch, size_t scratch_bytes,
                               mobocmf_stream_t stream);

/* GPyTorch's shortcut branch (inputs identical to the inducing inputs: q(u) itself): the marginal
 * variances var[i] = max(sum_{j<=i} L_S[i][j]^2, min_var) of S = L_S L_S^T (L_S M x M row-major, lower triangle read), and
 * the gradient g_LS[i][j] = 2 L_S[i][j] g_var[i] (j <= i, var[i] above the floor; 0 elsewhere). */
int mobocmf_shortcut_var_forward(const double* L_S, int32_t M, double min_var, double* var, mobocmf_stream_t stream);
int mobocmf_shortcut_var_backward(const double* L_S, const double* var, const double* g_var, int32_t M, double min_var,
                                  double* g_LS, mobocmf_stream_t stream);

/* ELBO tail (variational_elbo_mf.py:37-51): out2[0] = sum data_terms - scale * sum kls, out2[1] = scale * sum kls
 * (scale = batch / num_data).  Arrays of device-scalar pointers are HOST arrays, at most 8 entries each.
 * Backward: g2[0] = gradient w.r.t. every data term = g_elbo; g2[1] = w.r.t. every KL = scale * (g_skl - g_elbo);
 * g_elbo / g_skl are device scalars, either may be NULL (= 0). */
int mobocmf_elbo_combine_forward(int32_t n_data, const double* const* data_terms, int32_t n_kl, const double* const* kls,
                                 double scale, double* out2, mobocmf_stream_t stream);
int mobocmf_elbo_combine_backward(const double* g_elbo, const double* g_skl, double scale, double* g2,
                                  mobocmf_stream_t stream);

/* The whole ELBO of variational_elbo_mf.py:24-51 in one call (a reduction launch + a one-block tail; the same in backward;
 * the per-fidelity functions above take two launches per fidelity + mobocmf_elbo_combine): for every layer l < L with mean[l]
 * non-NULL the masked expected log-likelihood of the rows with fid == l (mean[l] / var[l] hold B * div[l] rows, row i belongs
 * to y[i / div[l]]; averaged over the div[l] samples of a row), noise tau_l = lo[l] + (hi[l] - lo[l]) sigmoid(raw_noise[l][0])
 * (hi[l] <= lo[l]: raw_noise[l][0] is tau itself); n_kl KL scalars; scale = batch / num_data:
 *   out3[0] = sum data terms - scale * sum kls,  out3[1] = scale * sum kls,  out3[2] = -out3[0]  (the loss).
 * rows (HOST array of L entries, or NULL = B everywhere): layer l holds only the FIRST rows[l] <= B rows of the batch
 * (rows[l] * div[l] entries).  The reference evaluates every layer at every row and then masks (:33-38); a row of fidelity
 * f reaches the loss only through layers 0..f, so with the batch ordered by descending fidelity layer l needs the prefix
 * of rows with fidelity >= l and nothing else (mobocmf_amd.util.graphed_step orders the batch this way once).
 * Arrays of pointers / per-layer values are HOST arrays of L (n_kl) entries, L, n_kl <= 8.  scratch >= 8 * 512 * 8 bytes.  Backward: g_mean[l] / g_var[l] (B * div[l]), g_raw_noise[l] (w.r.t. the RAW parameter; may be
 * NULL per layer), g_kl[0] = the gradient w.r.t. every KL = scale * (g_skl - g_elbo); g_elbo / g_skl device scalars or NULL. */
int mobocmf_elbo_forward(int32_t L, const double* const* mean, const double* const* var, const int32_t* div,
                         const double* const* raw_noise, const double* lo, const double* hi, const double* y,
                         const double* fid, int64_t B, const int64_t* rows, int32_t n_kl, const double* const* kls, double scale,
                         double* out3, void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);
int mobocmf_elbo_backward(int32_t L, const double* const* mean, const double* const* var, const int32_t* div,
                          const double* const* raw_noise, const double* lo, const double* hi, const double* y,
                          const double* fid, int64_t B, const int64_t* rows, double scale, const double* g_elbo,
                          const double* g_skl, double* const* g_mean, double* const* g_var, double* const* g_raw_noise,
                          double* g_kl, void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);

/* The same pair with the noise given as the RAW parameter of an Interval constraint (mfdgp.py:116):
 * tau = lo + (hi - lo) * sigmoid(raw_noise[0]) is evaluated inside the kernels and g_tau is the gradient w.r.t. the raw
 * parameter (hi <= lo: raw_noise is taken as tau itself, i.e. the plain functions above). */
int mobocmf_elbo_data_interval_forward(const double* mean, const double* var, const double* y, const double* fid,
                                       const double* raw_noise, double lo, double hi, double level, int64_t n_rows,
                                       int32_t div, double* out, void* scratch, size_t scratch_bytes,
                                       mobocmf_stream_t stream);
int mobocmf_elbo_data_interval_backward(const double* mean, const double* var, const double* y, const double* fid,
                                        const double* raw_noise, double lo, double hi, double level, int64_t n_rows,
                                        int32_t div, const double* g_out, double* g_mean, double* g_var, double* g_tau,
                                        void* scratch, size_t scratch_bytes, mobocmf_stream_t stream);

/* mus[t] = mean_s mu~[t*S+s];  vars[t] = mean_s(var~ + mu~^2) - mus^2   (mfdgp.py:258-260). */
int mobocmf_acq_moments_forward(const double* mu_t, const double* var_t, double* mus, double* vars, int64_t T,
                                int32_t S, mobocmf_stream_t stream);
int mobocmf_acq_moments_backward(const double* mu_t, const double* g_mus, const double* g_vars, double* g_mu_t,
                                 double* g_var_t, int64_t T, int32_t S, mobocmf_stream_t stream);
/* acq[t] = 0.5 * max(log v_uncond[t] - log v_cond[t], 0)   (JESMOC_MFDGP.py:52). */
int mobocmf_jes_forward(const double* v_uncond, const double* v_cond, double* acq, int64_t T, mobocmf_stream_t stream);

/* Fused Adam update (torch.optim.Adam defaults: no weight decay, no amsgrad) of one flat parameter
 * segment; `step` is the 1-based step count.  mask (may be NULL) = 0 freezes an element. */
int mobocmf_adam_step(double* param, const double* grad, double* exp_avg, double* exp_avg_sq, const double* mask,
                      int64_t n, double lr, double beta1, double beta2, double eps, int64_t step,
                      mobocmf_stream_t stream);

/* The same update for ALL parameter tensors of a model in one launch (<= 40 tensors per launch; more are chunked).
 * The arrays of pointers / sizes are HOST arrays (copied into the kernel arguments, so a captured graph replays them);
 * step_state is ONE device int64 holding the number of completed steps: the launch uses step_state[0] + 1 for the bias
 * corrections and a trailing one-thread launch increments it (no host-side step count: capturable).  Tensors without a
 * gradient are simply left out by the caller. */
int mobocmf_adam_multi(int32_t n_tensors, double* const* params, const double* const* grads, double* const* exp_avg,
                       double* const* exp_avg_sq, const int64_t* sizes, double lr, double beta1, double beta2, double eps,
                       int64_t* step_state, mobocmf_stream_t stream);

/* Constrained hyper-parameters of a layer in one launch: out = softplus of n_tensors raw parameter tensors (HOST arrays of
 * device pointers / sizes, copied into the kernel arguments: capturable), concatenated in the given order -- the `hyp`
 * vector of mobocmf_layer_forward built from GPyTorch's raw_outputscale / raw_lengthscale / raw_variance parameters with
 * their Positive() constraints (gpytorch.constraints.Positive = softplus; mfdgp_hidden_layer.py:43-47,68-88).  The
 * backward writes one gradient tensor per raw tensor.  n_tensors <= 16. */
int mobocmf_softplus_pack(int32_t n_tensors, const double* const* raw, const int32_t* sizes, double* out,
                          mobocmf_stream_t stream);
int mobocmf_softplus_pack_backward(int32_t n_tensors, const double* const* raw, const int32_t* sizes, const double* g_out,
                                   double* const* g_raw, mobocmf_stream_t stream);
/* The same with one upstream-gradient pointer PER TENSOR (g_out[i]: sizes[i] doubles, NULL = zero): for a caller that packs
 * the hyper-parameters of several layers in one launch and hands the segments out as separate tensors. */
int mobocmf_softplus_pack_backward_v(int32_t n_tensors, const double* const* raw, const int32_t* sizes,
                                     const double* const* g_out, double* const* g_raw, mobocmf_stream_t stream);

/* ---- Conditioned training: the theta / omega factor losses of blackbox_mfdgp_fitter.py:227-243 and the glue
 * around them -- a few hundred flops that cost ~100 framework launches per iteration of a launch-bound loop.
 *
 * mobocmf_cond_factors_forward:  loss[0] = sum_{p < P, t < T} [ coef_c c(p,t) + coef_1mc (1 - c(p,t)) ] with
 *   c(p,t) = prod_k Phi((cs_mean[k][t] - thresholds[k]) / sqrt(cs_var[k][t]))
 *          * prod_j Phi((pareto_front[p][j] - fs_mean[j][t]) / sqrt(fs_var[j][t]))
 *   (n_obj, n_con <= 8; one row pointer per objective / constraint, T entries each; pareto_front [P x n_obj] row-major).
 *   omega factors (:235-243): coef_c = log eps, coef_1mc = log(1 - eps), P = Pareto points, T = the x~ points.
 *   theta factors (:227-233): n_obj = 0, n_con = 1, P = 1, T = Pareto points, coef_c = log(1 - eps), coef_1mc = log eps.
 *   g_*: d loss / d (every input entry) for an upstream gradient of 1, formed in the same launch.
 * mobocmf_scale_segments:   out_i[e] = g[0] * coef_i * in_i[e]   (g: device scalar, NULL = 1; coef NULL = 1): the backward of
 *   anything whose forward formed its own gradient.
 * mobocmf_gather_segments:  out = segments back to back, zeros where in[i] is NULL: the backward of a split into row ranges.
 * mobocmf_scalar_combine:   out[0] = sum_i coef[i] * x[i][0]: a loss assembled from scalar terms (coef: HOST array).
 * n <= 32 segments; sizes / coef are HOST arrays. */
int mobocmf_cond_factors_forward(int32_t n_obj, int32_t n_con, int32_t P, int32_t T, const double* const* fs_mean,
                                 const double* const* fs_var, const double* const* cs_mean, const double* const* cs_var,
                                 const double* pareto_front, const double* thresholds, double coef_c, double coef_1mc,
                                 double* loss, double* const* g_fs_mean, double* const* g_fs_var, double* const* g_cs_mean,
                                 double* const* g_cs_var, mobocmf_stream_t stream);
int mobocmf_scale_segments(int32_t n, const double* const* in, double* const* out, const int64_t* sizes, const double* coef,
                           const double* g, mobocmf_stream_t stream);
int mobocmf_gather_segments(int32_t n, const double* const* in, const int64_t* sizes, double* out, mobocmf_stream_t stream);
int mobocmf_scalar_combine(int32_t n, const double* const* x, const double* coef, double* out, mobocmf_stream_t stream);

/* ---- The whole ELBO step of SMALL surrogates in ONE launch (blackbox_mfdgp_fitter.py:161-171 at the reference's own sizes:
 * M = N = tens of points, examples/example_acquisition_mfdgp_forrester/...py:51-62).  At those sizes a step through the layer
 * entry points above is ~50 dependent launches of ~4.7 us each whatever they compute.  Here ONE workgroup per surrogate runs
 * zero_grad + MFDGP.forward + VariationalELBOMF + backward + Adam (torch.optim.Adam semantics) as a sequence of
 * workgroup-barrier-separated phases: the M x M chain lives in LDS, the M x N' panels in `work`; several surrogates = several
 * workgroups of the same launch.  Same algebra and the same results as the layer path, rows ordered by DESCENDING
 * fidelity with layer l evaluated on the first rows[l] of them.
 *
 * Limits: L <= 3 layers, M <= 32 inducing points shared by all layers (Z~_l = [Zx, m_{l-1}], mfdgp_hidden_layer.py:555-556),
 * d <= 8, train branch only.  mobocmf_tiny_model is read by the kernel from DEVICE memory (`dev_models`: the caller uploads the
 * array once); `host_models` is the same array in host memory, used for validation and launch geometry only.
 *   raw[l][s]: the raw (unconstrained, softplus) kernel parameters in the packed order of the hyper-parameter vector above --
 *     layer 0: s = 0 outputscale (1), s = 1 lengthscales (d); layers >= 1: s = 0..4 a1, af, nu, a2, lsf (1 each), s = 5 ls1 (d),
 *     s = 6 ls2 (d).  m[l] (M), L_S[l] (M x M row-major, lower triangle used), raw_noise[l] (Interval(noise_lo, noise_hi)).
 *   trainable[l]: bit s (< 7) raw[l][s], bit 7 m, bit 8 L_S, bit 9 raw_noise -- cleared bits are left untouched by the update.
 *   rng[l] (l >= 1): {seed, calls, ticket} of the layer's eps stream as in mobocmf_propagate_rng_forward (same draws for the
 *     same state; `calls` advances by one per step); eps[l] != NULL replaces the draw (rows[l] * S values).
 *   Flat layout of grad / adam_m / adam_v (mobocmf_tiny_flat_len doubles): per layer [packed hyper-parameters | m | L_S], then
 *     raw_noise of every layer.  grad (optional) receives d(-ELBO)/d(raw parameters) of the step.
 *   out[0] = ELBO, out[1] = scaled KL, out[2] = -ELBO (before the update); info[l] = 0 or the failed Cholesky pivot (1-based).
 * do_update is one of the MOBOCMF_STEP_* modes below.  GRADIENTS: gradients only (no parameter, optimiser or rng-counter
 * write); UPDATE: the step; FORWARD: forward only (out, top_mean / top_var; draws the random rows of x) -- a conditioned
 * iteration is FORWARD, the factor launches on top_mean / top_var, UPDATE; INPUT_GRADIENTS: the parameters are constants
 * (acquisition search, JESMOC_MFDGP.py:38-52): `grad` receives d / d x (N x d) of <seed_gmean, top mean> + <seed_gvar, top var>
 * (times seed_scale) and nothing else is written -- predictive moments of fitted models are FORWARD with branch = 1, eps[l] =
 * the layer's fixed samples tiled over the test points; COUPLED: UPDATE with the factor terms of the conditioned loss formed
 * INSIDE the launch (mobocmf_tiny_coupling: ONE launch per conditioned iteration instead of FORWARD + factor launches + UPDATE). */
#define MOBOCMF_STEP_GRADIENTS 0
#define MOBOCMF_STEP_UPDATE 1
#define MOBOCMF_STEP_FORWARD 2
#define MOBOCMF_STEP_INPUT_GRADIENTS 3
#define MOBOCMF_STEP_COUPLED 4
#define MOBOCMF_TINY_MAX_LAYERS 3
#define MOBOCMF_TINY_MAX_M 32
#define MOBOCMF_TINY_MAX_D 8
typedef struct mobocmf_tiny_model {
    int32_t L, M, d, S;
    int32_t N;                               /* batch rows, ordered by descending fidelity */
    int32_t rows[MOBOCMF_TINY_MAX_LAYERS];   /* rows[0] == N >= rows[1] >= ... >= 1 */
    uint32_t trainable[MOBOCMF_TINY_MAX_LAYERS];
    int32_t branch;                          /* 0: train branch (clamp(k_nn - q, 0)), 1: eval branch (no clamp), as the layers */
    const double* x;                         /* N x d */
    const double* y;                         /* N */
    const double* fid;                       /* N (levels as doubles, as VariationalELBOMF compares them) */
    const double* Zx;                        /* M x d */
    double* raw[MOBOCMF_TINY_MAX_LAYERS][7];
    double* m[MOBOCMF_TINY_MAX_LAYERS];
    double* L_S[MOBOCMF_TINY_MAX_LAYERS];
    double* raw_noise[MOBOCMF_TINY_MAX_LAYERS];
    double noise_lo[MOBOCMF_TINY_MAX_LAYERS], noise_hi[MOBOCMF_TINY_MAX_LAYERS];
    int64_t* rng[MOBOCMF_TINY_MAX_LAYERS];
    const double* eps[MOBOCMF_TINY_MAX_LAYERS];
    double* adam_m;
    double* adam_v;
    int64_t* steps_done;                     /* completed Adam steps (device word, advanced by the launch) */
    double* work;                            /* mobocmf_tiny_work_bytes */
    double* grad;                            /* optional */
    double* out;                             /* 3 doubles */
    int32_t* info;                           /* L words */
    double kl_scale;                         /* d loss / d KL_l: batch / num_data (variational_elbo_mf.py:44-47) */
    double jitter;
    /* Conditioned training (blackbox_mfdgp_fitter.py:270-343), all optional (NULL / 0: the plain ELBO step).  The loss of a
     * model is  -sum_rows row_weight[b] E_q[log p(y_b | f)] + kl_scale sum_l KL_l  + <seeds, top-layer moments>: rows scored
     * with another weight (the batch term's num_data / B, a Pareto point's 1) or not at all (weight 0: x~ rows, the Pareto
     * rows of a constraint), and gradients of terms formed OUTSIDE the launch (the theta / omega factors,
     * mobocmf_cond_factors_forward) entering at the top layer's columns. */
    const double* row_weight;                /* N (NULL: 1) */
    const double* seed_gmean;                /* rows[L-1] * S: d(outside term) / d mean of the top layer's columns (NULL: none;
                                              * MOBOCMF_STEP_COUPLED WRITES both arrays itself before its backward reads them) */
    const double* seed_gvar;
    double seed_scale;                       /* the outside term's coefficient in the loss (the fitter's -1) */
    double* top_mean;                        /* rows[L-1] * S: the top layer's moments, written by every mode (NULL: not) */
    double* top_var;
    int64_t* xrng;                           /* {seed, calls}: FORWARD / COUPLED draw rows [rand_row0, rand_row0 + rand_rows) of x from */
    int32_t rand_row0, rand_rows;            /* U(0,1) (the x~ of :276; x must be writable); UPDATE / COUPLED of model 0 advance calls */
    /* MOBOCMF_STEP_COUPLED (the whole conditioned iteration in ONE launch with an in-launch barrier): what couples the models, and this model's part in it */
    const struct mobocmf_tiny_coupling* coupling;
    int32_t role, role_index;                /* 0: objective role_index of the coupling, 1: constraint role_index */
} mobocmf_tiny_model;
/* The theta / omega factors of blackbox_mfdgp_fitter.py:227-243 over the models of one launch (device-resident, shared).
 * Every model holds, at its TOP layer with S = 1, the P Pareto points in columns [0, P) and the T points x~ in [P, P + T).
 * After its forward every workgroup publishes its top-layer moments, the workgroups of the launch meet at a barrier (an arrival
 * counter in device memory -- an ordinary launch, not a cooperative one: mobocmf_tiny_elbo_step checks n_models against the
 * device's occupancy for the kernel, n_models <= 64, 1 <= T <= 256), and every workgroup forms the factor gradients of ITS model -- the omega factors from all models' moments at x~, a constraint's theta
 * factors from its own at the Pareto points -- into its seed_gmean / seed_gvar before running its backward and update. */
typedef struct mobocmf_tiny_coupling {
    int32_t n_obj, n_con, P, T;
    int32_t obj_model[8], con_model[8];      /* index in the launch's model array of every objective / constraint */
    const double* front;                     /* P x n_obj (Pareto front, columns in objective order) */
    const double* thresholds;                /* n_con */
    double log_eps, log_1m_eps;
    double* losses;                          /* n_con + 1: the theta factor term of every constraint, then the omega term */
    int64_t* barrier;                        /* device word: arrivals at the in-launch barrier.  Monotonic: launch k of the record
                                              * waits for k * n_models arrivals, so ONE record serves ONE launch at a time
                                              * (launches of a record are ordered on one stream) and always with the same n_models */
    int32_t* status;                         /* device word, only ever OR'd by the launches: bit 0 a workgroup gave up waiting at
                                              * the barrier, bit 1 the launch did not match the record (n_models, T, P).  The
                                              * caller zeroes barrier and status together, once before the first launch and
                                              * again only after reading a non-zero status (the in-launch wait contract:
                                              * mobocmf_check_info) */
    int32_t n_models;                        /* workgroups (= models) of the launches this record is for; the kernel checks */
    int32_t reserved;
} mobocmf_tiny_coupling;
int mobocmf_tiny_flat_len(const mobocmf_tiny_model* model, int64_t* len);
int mobocmf_tiny_work_bytes(const mobocmf_tiny_model* model, size_t* bytes);
int mobocmf_tiny_elbo_step(const mobocmf_tiny_model* host_models, const mobocmf_tiny_model* dev_models, int32_t n_models,
                           double lr, double beta1, double beta2, double eps, int32_t do_update, mobocmf_stream_t stream);

/* ---- The same step for MID-SIZE surrogates (M <= 128 inducing points: the reference's own BO loop runs M = N from 15 to 75,
 * examples/toy_synthetic_2D_JESMOCMF/toy_synthetic_2D_JESMOCMF.py:25,102-103,305-331 with mfdgp.py:295-298; BASELINE config 2 has
 * M = 128), still ONE launch per step for a whole group of surrogates, by SEVERAL workgroups per surrogate: the step is ~11
 * phases separated by an in-launch barrier of the surrogate's workgroups (arrival counter + agent-scope fences); every product
 * runs on v_mfma_f64_16x16x4_f64.  Same descriptor (mobocmf_tiny_model; M <= MOBOCMF_COOP_MAX_M, d <= 8, L <= 3), same flat
 * layout of grad / adam_m / adam_v (mobocmf_tiny_flat_len), same draws, same results as the layer path up to summation order;
 * `work` is sized by mobocmf_coop_work_bytes.  do_update: MOBOCMF_STEP_GRADIENTS | UPDATE | FORWARD | INPUT_GRADIENTS
 * (as mobocmf_tiny_elbo_step's: `grad` <- N x d, d/dx of <seed_gmean, top mean> + <seed_gvar, top var>; needs `grad`
 * and the seeds; nothing else is written) | COUPLED, the conditioned iteration in one launch (mobocmf_tiny_coupling with n_models = the models of the launch; the barrier of its record is not
 * used: the whole grid meets on the launch's own sync words).
 * wgs_per_model: workgroups sharing one surrogate, 1..64, or 0 = chosen from the widest phase (at most 32); *wgs_used (may be
 * NULL) receives the choice.  Every workgroup of the launch must be resident at once (n_models * wgs_per_model <= what the
 * device holds of this kernel: checked, MOBOCMF_BAD_ARG otherwise -- an ordinary launch, not a cooperative one, so that it can
 * be captured into a graph).  sync_words: 16 * (n_models + 1) device int64 -- monotonic arrival counters (a group of words
 * serves one launch at a time, always with the same wgs_per_model and n_models) and, at word 16 * n_models + 1, the status
 * word of the in-launch wait contract (mobocmf_check_info; bit 0 a wait gave up, bit 1 MOBOCMF_STEP_COUPLED did not match its coupling
 * record).  The caller zeroes the block once before the first launch and again only after reading a non-zero status; a
 * workgroup that gives up also sets info[0] = -1 and out[2] = NaN. */
#define MOBOCMF_COOP_MAX_M 128
/* OR'd into MOBOCMF_STEP_FORWARD or MOBOCMF_STEP_INPUT_GRADIENTS of mobocmf_coop_elbo_step: the parameters are the ones of an earlier launch on the same `work`
 * (an acquisition search against fitted models, JESMOC_MFDGP.py:137-184): K_mm, its Cholesky and inverse, U, a and the KL stay as
 * that launch left them and are not formed again (35-65 us of a ~140 us launch).  The caller vouches for it. */
#define MOBOCMF_STEP_CHAIN_VALID 16
int mobocmf_coop_work_bytes(const mobocmf_tiny_model* model, size_t* bytes);
int mobocmf_coop_elbo_step(const mobocmf_tiny_model* host_models, const mobocmf_tiny_model* dev_models, int32_t n_models,
                           int32_t wgs_per_model, int64_t* sync_words, double lr, double beta1, double beta2, double eps,
                           int32_t do_update, int32_t* wgs_used, mobocmf_stream_t stream);

/* ---- Exact-GP comparison baselines (mobocmf/models/mfgp.py:24-141,145-184; mfgp_lin.py:101-189) on the layer's kernels.
 * The reference inherits exact inference from GPyTorch's ExactGP; here the Gram matrices come from mobocmf_gram_forward,
 * the multi-fidelity combination is one element-wise launch, the factorisation / triangular inverse are the variational
 * layer's (blocked Cholesky + MFMA), the predictive moments its triangular product with the column-statistics epilogue.
 *
 * mobocmf_mf_kernel_combine: out[i][j] = s1[i] s2[j] Ks[i][j] + ntab[min(l1[i], l2[j])] Kn[i][j] (+ diag if i == j), i < n1,
 *   j < n2; zero (identity on the diagonal when diag != 0) in the padding up to rows_p x cols_p.  Ks / Kn: the two ARD-RBF Gram
 *   matrices (signal / noise kernel, ld), l1 / l2 int32 fidelity levels, s1 / s2 per-row / per-column signal factors (NULL = 1),
 *   ntab[level] the noise factor (MFKernel: the level itself; MFKernel_lin: its rho polynomial).
 * mobocmf_exact_gp_factor: K = the n x n training covariance with the noise on its diagonal; leaves L, L^-1, a = L^-1 y in
 *   `state`, mll[0] = log N(y | 0, K), info = 0 or the failed pivot.
 * mobocmf_exact_gp_predict: mean[j] = k_j^T K^-1 y, var[j] = kss[j] - k_j^T K^-1 k_j for the nt columns k_j of Kts [n x nt].
 * Sizes from mobocmf_exact_gp_workspace_bytes (state for a given n; scratch for n and up to nt test points per call). */
int mobocmf_mf_kernel_combine(int64_t n1, int64_t n2, const double* Ks, const double* Kn, int64_t ld, const double* s1,
                              const double* s2, const int32_t* l1, const int32_t* l2, const double* ntab, double diag,
                              double* out, int64_t ldo, int64_t rows_p, int64_t cols_p, mobocmf_stream_t stream);
int mobocmf_exact_gp_workspace_bytes(int32_t n, int64_t nt, size_t* state_bytes, size_t* scratch_bytes);
int mobocmf_exact_gp_factor(int32_t n, const double* K, int64_t ldk, const double* y, double* mll, int32_t* info, void* state,
                            size_t state_bytes, void* scratch, size_t scratch_bytes, const mobocmf_tuning* tuning,
                            mobocmf_stream_t stream);
int mobocmf_exact_gp_predict(int32_t n, int64_t nt, const double* Kts, int64_t ld, const double* kss, double* mean,
                             double* var, const void* state, size_t state_bytes, void* scratch, size_t scratch_bytes,
                             const mobocmf_tuning* tuning, mobocmf_stream_t stream);

/* The f64 MFMA GEMM used by the layer (exposed for tests and for the roofline measurement of bench.py):
 * C[Mr x Nc] (+)= alpha * A[Mr x Kd] * B, B is [Kd x Nc] (trans_b = 0) or [Nc x Kd] (trans_b = 1).
 * Mr, Nc multiples of 128, Kd multiple of 16, leading dimensions even, pointers 16-byte aligned.  Other sizes are accepted
 * only where a kernel that handles them takes the product under the given tuning, MOBOCMF_BAD_ARG otherwise: all three
 * multiples of 16 and <= tuning.small_gemm_max (small-operand kernel); Mr, Nc multiples of 64 and Kd of 32, all <=
 * tuning.mid_gemm_max (mid-size kernel); A B form with Mr, Kd multiples of 128 and <= tuning.small_panel_max, B not
 * triangular and Nc any multiple of 16 with (Nc / 16) (Mr / 128) <= 512 (whole-block panel kernel).
 * tri: bit 0 A lower-triangular, bit 1 A upper-triangular, bit 2 B lower, bit 3 B upper (square operands; for B the flag
 * names the triangle of the logical Kd x Nc operand, whichever way it is stored).
 * Triangular-operand contract: the UNUSED TRIANGLE MUST HOLD ZEROS.  The flags only let a kernel skip work: with the operand
 * cut into 128 x 128 blocks from its origin, a block that lies wholly in the unused triangle (strictly beyond the block
 * diagonal) is never read and may hold anything; the blocks on the diagonal are read whole, and an entry of the unused
 * triangle inside them enters the product as stored.  (The small-operand kernels happen to mask those entries on load, the
 * mid-size and tiled kernels multiply them; which kernel runs is a matter of the tuning thresholds, so no caller may count
 * on the masking.  Every triangular operand of the layer -- L^-1, U, their transposes, dU, dL -- is stored with its zeros.)
 * The same holds for the triangular A of mobocmf_gemm_f64_epilogue.
 * tuning: NULL = defaults (the small / mid-size operand thresholds decide which kernel a product runs on). */
int mobocmf_gemm_f64(int32_t tri, int32_t trans_b, int32_t Mr, int64_t Nc, int64_t Kd, const double* A, int64_t lda,
                     const double* B, int64_t ldb, double* C, int64_t ldc, double alpha, int32_t accumulate,
                     const mobocmf_tuning* tuning, mobocmf_stream_t stream);

/* The same kernel with the epilogues the layer launches it with (tests, and bench.py's per-variant roofline):
 *   epi 0  plain store (dK = L^-T dA);
 *   epi 1  store + partial column statistics, mobocmf_gemm_colstat_rows() partial rows of Nc entries each (two per row
 *          block of the tile height the launch uses): sum_p colsq_part[p][n] =
 *          sum_i C[i][n]^2 and (coldot_part non-NULL) sum_p coldot_part[p][n] = sum_i avec[i] C[i][n]   (A = L^-1 K -> q,
 *          mean; C = U^T A -> r);
 *   epi 2  C[i][n] = alpha bscale[n] (A B)[i][n] + avec[i] gmu[n] - 2 Aaux[i][n] cgv[n]   (dA), and (rowdot_part
 *          non-NULL) rowdot_part[slice][i] = partial sums over 64-column slices of Aaux[i][n] gmu[n]   (da).
 * B is [Kd x Nc] (no transposed form).  stream_out: non-temporal stores of C.  Pointers an epilogue does not use: NULL.
 * col_activity (NULL = dense): DEVICE array of one int32 per 128 columns of C; the column blocks marked 0 are left unwritten
 * (their row-dot partials zeroed) -- how the tests drive the block skipping of the layer backward directly.  The tile
 * height / pairing come from `tuning`.  Where the whole-block panel kernel takes the product (A B form, Mr and Kd multiples
 * of 128 and <= tuning.small_panel_max, at most 512 workgroups of 128 rows x 16 columns) Nc may be any multiple of 16; it then
 * writes Nc / 16 row-dot partial rows, the tiled kernel 2 * (Nc / 128).  col_activity then holds one word per STARTED 128
 * columns, ceil(Nc / 128) words: the last word governs the partial block. */
int mobocmf_gemm_f64_epilogue(int32_t tri, int32_t epi, int32_t Mr, int64_t Nc, int64_t Kd, const double* A, int64_t lda,
                              const double* B, int64_t ldb, double* C, int64_t ldc, double alpha, int32_t stream_out,
                              double* colsq_part, double* coldot_part, const double* avec, const double* bscale,
                              const double* gmu, const double* cgv, const double* Aaux, double* rowdot_part,
                              const int32_t* col_activity, const mobocmf_tuning* tuning, mobocmf_stream_t stream);

/* Partial rows an epi-1 launch of that shape writes to colsq_part / coldot_part under the same `tuning` (tile height). */
int mobocmf_gemm_colstat_rows(int32_t tri, int32_t Mr, int64_t Nc, int64_t Kd, const mobocmf_tuning* tuning, int32_t* rows);

/* The weighted symmetric rank-k update of the layer backward, H[Mr x Mr] = A diag(w) A^T with A [Mr x Kd] (k contiguous,
 * lda even) and w [Kd]: k-sliced over one round of resident workgroups into slabs (workspace), the slabs added and the
 * result written as the FULL symmetric matrix.  Both M x M contractions over N' of the reference's autograd backward
 * (A diag(gv) C^T for dU and dA K^T for dL^-1) reduce to it.  Mr, Kd multiples of 128.
 * k_activity (NULL = dense): DEVICE array of one int32 per 128 entries of the contraction; the blocks marked 0 (w is zero
 * throughout them) are left out.  The size query and the launch take the same `tuning` (syrk_workgroups sets the slab count). */
int mobocmf_syrk_workspace_bytes(int32_t Mr, int64_t Kd, const mobocmf_tuning* tuning, size_t* bytes);
int mobocmf_syrk_weighted_f64(int32_t Mr, int64_t Kd, const double* A, int64_t lda, const double* w, double* H,
                              void* workspace, int64_t workspace_bytes, const int32_t* k_activity,
                              const mobocmf_tuning* tuning, mobocmf_stream_t stream);

/* Host-side, synchronising: copies the device word and returns MOBOCMF_OK or MOBOCMF_NOT_PD (pivot in *pivot: the 1-based
 * column of the first non-positive pivot; -1 = a one-launch form abandoned a bounded in-launch wait because its workgroups
 * were not resident together: the results of that call are invalid, repeat it with less concurrent work or with the
 * launch-per-step form).
 * The in-launch wait contract of the one-launch forms (the one-launch Cholesky, mobocmf_tuning.potrf_cols = 0; the cooperative
 * step; MOBOCMF_STEP_COUPLED of mobocmf_tiny_elbo_step): they are ordinary launches whose workgroups wait for each other, so the host checks
 * that all of them are resident at once, and every wait is bounded by 1 s of the device's wall clock.  A give-up is reported
 * only by an atomic OR into a status word, which no later workgroup or launch clears, and every wait releases only while that
 * word is zero.  Where the counters persist across launches (sync_words of mobocmf_coop_elbo_step, the barrier / status of
 * mobocmf_tiny_coupling) every later wait then fails at its first poll, so nothing commits parameters, optimiser state, step
 * counts or random streams until the caller has read the status and zeroed counters and status together.  The one-launch
 * Cholesky zeroes its words before every launch; its closing launch turns a set status into info = -1 and NaN on the diagonals
 * of the factor and of the inverse, so that anything computed from them is non-finite even after info is rewritten. */
int mobocmf_check_info(const int32_t* info, int32_t* pivot, mobocmf_stream_t stream);

/* Natural-gradient step of the variational distributions q(u) = N(m, L_S L_S^T) of n layers of equal M, in place (DESIGN.md,
 * "Natural gradients"): with G_S = dloss/dS obtained from g_LS by the reverse-mode Cholesky rule,
 *     S_new^-1 = S^-1 + 2 gamma_t scale G_S,     m_new = m - gamma_t scale S_new g_m,
 * returned as L_new = L_S T (lower triangular, the diagonal signs of L_S kept) with T T^T = (I + 2 gamma_t scale Psi)^-1,
 * Psi = sym(Phi(L_S^T g_LS)).  g_m [M] and g_LS [M x M] are the gradients of the caller's loss; `scale` is what turns that loss
 * into -ELBO (num_data / batch rows for a loss of the form data terms summed over the batch - (batch / num_data) KL: 1 on the
 * full batch), so that gamma = 1 is the exact conjugate step.  Of L_S and g_LS
 * (row-major, ld M) only the lower triangle is read, and only the lower triangle of L_S is written.
 * Schedule, evaluated on the device: gamma_t = min(gamma, gamma_init (gamma / gamma_init)^(t / warmup_steps)) with t =
 * step_count[0] (ONE device int64, which the call increments); warmup_steps = 0: gamma_t = gamma.
 * Failure rule: info[z] (device int32, one per layer) receives the pivot report of the factorisation of I + 2 gamma_t scale Psi
 * (0 = positive definite; the contract of mobocmf_check_info, -1 = abandoned in-launch wait included).  A layer with info != 0
 * keeps its m and L_S bitwise and skipped[z] (device int32, one per layer, caller-zeroed) is incremented; the step counter
 * advances all the same.  Nothing is read on the host: capturable.  Two calls on the same inputs give bitwise equal results.
 * Arrays of pointers are HOST arrays of n entries (device pointers inside).  workspace: mobocmf_natgrad_workspace_bytes(M, n)
 * bytes of device memory, 256-byte aligned.
 * MOBOCMF_BAD_ARG (host-visible, before any HIP call): a NULL pointer, n outside 1..4, M outside 1..MOBOCMF_NATGRAD_MAX_M,
 * gamma, gamma_init or scale not positive and finite, gamma_init > gamma, warmup_steps < 0, a malformed tuning record;
 * MOBOCMF_WORKSPACE_TOO_SMALL: bytes below the reported size. */
#define MOBOCMF_NATGRAD_MAX_M 1024
int mobocmf_natgrad_workspace_bytes(int32_t M, int32_t n, size_t* bytes);
int mobocmf_natgrad_step(int32_t n, int32_t M, double* const* m, double* const* L_S, const double* const* g_m,
                         const double* const* g_LS, double gamma, double gamma_init, int32_t warmup_steps, double scale,
                         int64_t* step_count, int32_t* const* skipped, int32_t* const* info, void* workspace, size_t bytes,
                         const mobocmf_tuning* tuning, mobocmf_stream_t stream);

/* ---- The same update for SMALL layers (M <= MOBOCMF_NATGRAD_SMALL_MAX_M), the sizes of the one-launch steps above: ONE launch
 * moves every layer of the array, one workgroup per layer, and M may differ from layer to layer (M <= 32: plain FP64 in LDS;
 * 32 < M <= 128: 16 x 16 tiles on v_mfma_f64_16x16x4_f64).  Meant as the second launch of a step whose first launch --
 * mobocmf_tiny_elbo_step / mobocmf_coop_elbo_step with `grad` set and the trainable bits 7 and 8 of the layer cleared -- left
 * d(-ELBO) / d m and / d L_S in its flat gradient: g_m and g_LS then point into that array.
 *   Algebra, schedule and failure rule are mobocmf_natgrad_step's: L_new = L_S T with T T^T = (I + 2 gamma_t scale Psi)^-1,
 *   m_new = m - gamma_t scale L_new L_new^T g_m, gamma_t = min(gamma, gamma_init (gamma / gamma_init)^(t / warmup_steps)).  Here
 *   EVERY layer has its own counter t = step_count[0] (device int64), read by its workgroup at entry and incremented at exit.
 *   A non-positive or non-finite pivot of J (I + 2 gamma_t scale Psi) J leaves m and L_S bitwise unchanged, writes the 1-based
 *   pivot to info[0] and increments skipped[0] (caller-zeroed); the counter advances all the same.  info[0] = 0 otherwise.
 *   Of L_S and g_LS (row-major, ld M) only the lower triangle is read; only the lower triangle of L_S is written; the diagonal
 *   signs of L_S are kept.
 *   Guard (all optional): guard_info / n_guard_info -- the info words of the launch that produced the gradients;
 *   guard_status -- the low 32 bits of that launch's in-launch status word (sync_words of mobocmf_coop_elbo_step, status of
 *   mobocmf_tiny_coupling); guard_loss -- its out[2].  If any of the words is non-zero or the loss is not finite, NOTHING of
 *   the layer is written -- m, L_S, step_count, skipped and info stay bitwise -- so that nothing commits parameters after a
 *   failed factorisation or an abandoned in-launch wait of the producing launch (mobocmf_check_info).
 *   work: mobocmf_natgrad_small_work_bytes(M) bytes of device memory owned by the layer (0 bytes, and NULL allowed, for
 *   M <= 32).  Two layers of one launch share nothing they write.
 * The kernel reads the records from DEVICE memory (`dev_layers`: the caller uploads the array once); `host_layers` is the same
 * array in host memory, used for validation and launch geometry only.  The launch waits for no other workgroup and has no
 * in-launch wait contract of its own; no atomics, fixed summation orders (two calls on the same inputs are bitwise equal);
 * nothing is read on the host: capturable.  The library keeps no state between calls.
 * MOBOCMF_BAD_ARG (host-visible, before any HIP call): host_layers or dev_layers NULL, n_layers < 1, and for any layer an M
 * outside 1..MOBOCMF_NATGRAD_SMALL_MAX_M, a NULL m, L_S, g_m, g_LS, step_count, skipped or info, a NULL work with M > 32, a
 * negative n_guard_info or a NULL guard_info with n_guard_info > 0, a scale that is not positive and finite; gamma or
 * gamma_init not positive and finite, gamma_init > gamma, warmup_steps < 0. */
#define MOBOCMF_NATGRAD_SMALL_MAX_M 128
typedef struct mobocmf_natgrad_small_layer {
    int32_t M;
    int32_t n_guard_info;                    /* words at guard_info (0: none) */
    double* m;                               /* M */
    double* L_S;                             /* M x M row-major, lower triangle used */
    const double* g_m;                       /* M: d loss / d m */
    const double* g_LS;                      /* M x M row-major, lower triangle used: d loss / d L_S */
    double scale;                            /* what turns the loss into -ELBO (mobocmf_natgrad_step) */
    int64_t* step_count;                     /* this layer's gamma-schedule counter */
    int32_t* skipped;                        /* one word, incremented when the step is skipped */
    int32_t* info;                           /* one word: 0 or the failed pivot */
    const int32_t* guard_info;               /* the producing launch's info words (may be NULL) */
    const int32_t* guard_status;             /* its in-launch status word (may be NULL) */
    const double* guard_loss;                /* its out[2] (may be NULL) */
    double* work;                            /* mobocmf_natgrad_small_work_bytes */
} mobocmf_natgrad_small_layer;
int mobocmf_natgrad_small_work_bytes(int32_t M, size_t* bytes);
int mobocmf_natgrad_small_step(const mobocmf_natgrad_small_layer* host_layers, const mobocmf_natgrad_small_layer* dev_layers,
                               int32_t n_layers, double gamma, double gamma_init, int32_t warmup_steps,
                               mobocmf_stream_t stream);

/* ---- The acquisition search on the device (csrc/acq_search.hip): the glue between the two one-launch model evaluations of an
 * iterate (mobocmf_tiny_elbo_step / mobocmf_coop_elbo_step, MOBOCMF_STEP_FORWARD then MOBOCMF_STEP_INPUT_GRADIENTS, over a predict
 * group whose models 2p / 2p + 1 are the unconditioned / conditioned surrogate of black-box p -- or, with K sampled Pareto sets,
 * whose models p (1 + K) .. p (1 + K) + K are the unconditioned and the K conditioned ones) and the selection of restarts and
 * winner -- the loop of optimize_acqf at mobocmf/acquisition_functions/JESMOC_MFDGP.py:137-184 with no host in it.  Each entry
 * point is ONE launch on `stream`, has no atomics and a fixed summation order (two calls on the same inputs are bitwise equal),
 * allocates nothing, reads nothing on the host and keeps no state: capturable.  A bad argument is refused with MOBOCMF_BAD_ARG
 * on the host, before any HIP call. */
#define MOBOCMF_ACQ_MAX_PAIRS 32
#define MOBOCMF_ACQ_MAX_COLUMNS (1 << 24) /* T * S */
#define MOBOCMF_TOPK_MAX_K 64
#define MOBOCMF_TOPK_MAX_N 4096

/* JES of every test point from the group's raw top-layer moments (JESMOC_MFDGP.py:38-52 over mfdgp.py:237-262): this IS
 * mobocmf_jes_mc_group_forward (below) with n_boxes = n_pairs and K = 1 -- the same launch, the same bits.
 *   moments  (2 n_pairs, 2, T S): per model its means then its variances WITHOUT noise, column t S + s
 *   noise    (2 n_pairs): the models' likelihood noise tau
 *   per model and test point, mbar = (1/S) sum_s mu_s:  v = (1/S) sum_s (var_s + tau + mu_s^2) - mbar^2   (S = 1: var + tau)
 *   acq[t] = sum_p 0.5 max(log v_{2p} - log v_{2p+1}, 0), summed in the order of p
 * want_seeds = 1: seeds (the layout of moments) = d (sum_t acq[t]) / d (raw mean, raw variance):  d a / d v_u = 0.5 / v_u and
 *   d a / d v_c = -0.5 / v_c where log v_u - log v_c >= 0, else 0 (equality passes, as torch.clamp's backward);
 *   d v / d var_s = 1 / S;  d v / d mu_s = 2 (mu_s - mbar) / S.
 * track = 1: wherever acq[t] > best_v[t] (strict; a NaN never wins) best_v[t] = acq[t] and row t of best_x (T x d) = row t of
 *   the iterate x (T x d); the caller fills best_v with -inf before the first call.
 * MOBOCMF_BAD_ARG: moments, noise or acq NULL; n_pairs outside 1..MOBOCMF_ACQ_MAX_PAIRS; T < 1; S < 1; T S >
 * MOBOCMF_ACQ_MAX_COLUMNS; a flag other than 0 / 1; want_seeds with seeds NULL; track with x, best_v or best_x NULL or d
 * outside 1..MOBOCMF_MAX_D. */
int mobocmf_jes_group_forward(const double* moments, const double* noise, int32_t n_pairs, int32_t T, int32_t S,
                              double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x, int32_t d,
                              double* best_v, double* best_x, mobocmf_stream_t stream);

/* JES averaged over K sampled Pareto sets (a Monte Carlo estimate of the information gain: the unconditioned surrogate of a
 * black-box is evaluated ONCE, against K surrogates conditioned on K different sampled Pareto sets).
 *   moments  (n_boxes (1 + K), 2, T S), noise (n_boxes (1 + K)): as above; model p (1 + K) is the unconditioned surrogate of
 *            black-box p, model p (1 + K) + 1 + k the one conditioned on sample k = 0 .. K - 1.  v and mbar per model as above.
 *   diff_pk = log v_u,p - log v_c,pk
 *   acq[t]  = sum_p (1 / K) sum_k 0.5 max(diff_pk, 0): the k-sum in the order of k, the product with 1 / K rounded, then the sum
 *             over p in the order of p.  A NaN stays a NaN.
 * want_seeds = 1: seeds (the layout of moments) = d (sum_t acq[t]) / d (raw mean, raw variance):
 *   d a / d v_c,pk = -0.5 / (K v_c,pk) where diff_pk >= 0, else 0;  d a / d v_u,p = #{k: diff_pk >= 0} 0.5 / (K v_u,p);
 *   d v / d var_s and d v / d mu_s as above.
 * track = 1: as above.
 * With K = 1 every expression is that of mobocmf_jes_group_forward with n_pairs = n_boxes (1.0 * the single term is exact),
 * which is this entry point at K = 1.
 * One launch of T workgroups of one wavefront: a lane per model, the sums by one lane in a fixed order, no atomics.
 * MOBOCMF_BAD_ARG: as for mobocmf_jes_group_forward, with n_boxes < 1, K < 1 or n_boxes (1 + K) > 2 MOBOCMF_ACQ_MAX_PAIRS in
 * place of its bound on n_pairs. */
int mobocmf_jes_mc_group_forward(const double* moments, const double* noise, int32_t n_boxes, int32_t K, int32_t T, int32_t S,
                                 double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x, int32_t d,
                                 double* best_v, double* best_x, mobocmf_stream_t stream);

/* JES per black-box, for decoupled evaluations (which black-box is evaluated next): moments, noise, the model layout (p (1 + K)
 * unconditioned, p (1 + K) + 1 + k conditioned), v, mbar and diff_pk exactly as for mobocmf_jes_mc_group_forward.
 *   term_p[t] = (1 / K) sum_k 0.5 max(diff_pk, 0): the k-sum in the order of k, the product with 1 / K rounded -- the summand of
 *               black-box p in mobocmf_jes_mc_group_forward's acq[t].  A NaN stays a NaN.
 * box_of_point == NULL (all boxes: the raw candidates are scored once for every black-box):
 *   acq[p acq_ld + t] = term_p[t] for p = 0 .. n_boxes - 1, acq_ld >= T the distance between two boxes' rows (a chunk of
 *   candidates writes its slice of an (n_boxes, n) array with acq_ld = n).  want_seeds and track must be 0.
 * box_of_point != NULL (T device words: the box each test point is searched for -- the replayed iterate), b = box_of_point[t]:
 *   acq[t] = term_b[t]; acq_ld is ignored.
 *   want_seeds = 1: the seeds (the layout of moments) of the 1 + K models of box b at the columns of t are d term_b[t] / d (raw
 *     mean, raw variance), the expressions of mobocmf_jes_mc_group_forward for those models (a model's seeds there depend on
 *     its own box only); the seeds of EVERY OTHER model at those columns are written as 0.0 in both arrays (never left stale:
 *     the MOBOCMF_STEP_INPUT_GRADIENTS launch that follows reads all of them).
 *   track = 1: as for mobocmf_jes_group_forward, on acq[t] = term_b[t].
 *   b outside [0, n_boxes) (the host cannot see the words): acq[t] = NaN, every seed at the columns of t 0.0, nothing tracked.
 * What ties it to mobocmf_jes_mc_group_forward on the same inputs, bit for bit (the two entry points are modes of ONE launch:
 * term_p and the seeds are formed by the same code in each, the modes differ in who sums and what is written):
 *   P1  sum_p acq[p acq_ld + t] of the all-box mode, accumulated in the order of p from 0.0, is that entry point's acq[t];
 *   P2  the selected-box acq[t] is the all-box acq[b acq_ld + t]; the seeds of box b's models are that entry point's seeds of
 *       those models; every other seed is 0.0;
 *   P3  n_boxes = 1 with all-zero words is that entry point in acq, seeds, best_v and best_x.
 * One launch of T workgroups of one wavefront: a lane per model, the lane of the unconditioned model of box p sums that box's K
 * terms in order; static LDS, no atomics, no wait on another workgroup.
 * MOBOCMF_BAD_ARG: as for mobocmf_jes_mc_group_forward; with box_of_point NULL also acq_ld < T, want_seeds != 0 or track != 0. */
int mobocmf_jes_mc_box_forward(const double* moments, const double* noise, int32_t n_boxes, int32_t K, int32_t T, int32_t S,
                               const int32_t* box_of_point, double* acq, int32_t acq_ld, int32_t want_seeds, double* seeds,
                               int32_t track, const double* x, int32_t d, double* best_v, double* best_x,
                               mobocmf_stream_t stream);

/* MES of every test point from the moments of exact-GP surrogates (the comparison baseline, MESMOC_MFGP: the expressions of
 * its _MES_MFGP.forward operation for operation), in the position mobocmf_jes_group_forward has in an iterate.
 *   moments  (n_obj + n_con, 2, T): per model its latent means then its variances, objectives first
 *   noise    (n_obj + n_con): the models' likelihood noise;   best (n_obj + n_con): best value per objective, threshold per
 *            constraint
 * With s = sqrt(var), z = (best - mean) / s, Phi(z) = 0.5 (1 + erf(z / sqrt 2)), phi(z) = exp(-z^2 / 2) / sqrt(2 pi), E = FLT_EPSILON:
 *   objective p:   cdf = min(Phi(z), 1 - E);  r = phi(z) / (1 - cdf);  vt = var max(1 + (z - r) r, E) + noise
 *                  term_p = max(0.5 log(var + noise) - 0.5 log(vt), 0)
 *   constraint c:  pf_c = 1 - Phi(z)
 *   acq[t] = (sum_p term_p, in the order of p) * (prod_c pf_c, in the order of c; 1 when n_con = 0)
 * A negative variance gives a NaN value.  want_seeds = 1: seeds (the layout of moments) = d acq[t] / d (mean, var) of every
 * model, the derivative automatic differentiation forms of the expressions above: each of the three clamps passes a gradient
 * where it does not bind (equality passes); under a binding min(., 1 - E) the cdf is a constant while phi still varies; a
 * constraint's seed carries the product over the OTHER constraints, formed explicitly in the order of c and never by division.
 * want_seeds = 0 gives the same acq bits.  track = 1: exactly the rule of mobocmf_jes_group_forward.
 * One launch of T workgroups of one wavefront: a lane per model, the sum and the products by one lane in a fixed order, no atomics.
 * MOBOCMF_BAD_ARG: moments, noise, best or acq NULL; n_obj < 1; n_con < 0; n_obj + n_con > 2 MOBOCMF_ACQ_MAX_PAIRS; T < 1 or
 * > MOBOCMF_ACQ_MAX_COLUMNS; a flag other than 0 / 1; want_seeds with seeds NULL; track with x, best_v or best_x NULL or d
 * outside 1..MOBOCMF_MAX_D. */
int mobocmf_mes_group_forward(const double* moments, const double* noise, const double* best, int32_t n_obj, int32_t n_con,
                              int32_t T, double* acq, int32_t want_seeds, double* seeds, int32_t track, const double* x,
                              int32_t d, double* best_v, double* best_x, mobocmf_stream_t stream);

/* One projected Adam ASCENT step on the iterate x (T x d): g[t][j] = -sum_i gx[i][t][j] over the n_models slices of the group's
 * input gradients gx (n_models, T, d) in the order of i, then the update of mobocmf_adam_multi (the same expressions in the same
 * order: with n_models = 1 the same bits) with the bias corrections of step steps_done[0] + 1, then x[t][j] clamped to
 * [lo[j], hi[j]].  steps_done is ONE device int64 (completed steps); the launch is one workgroup and advances it itself.
 * MOBOCMF_BAD_ARG: a NULL pointer; n_models outside 1..2 MOBOCMF_ACQ_MAX_PAIRS; T outside 1..MOBOCMF_TOPK_MAX_N; d outside
 * 1..MOBOCMF_MAX_D. */
int mobocmf_ascent_adam_step(double* x, const double* gx, int32_t n_models, int32_t T, int32_t d, const double* lo,
                             const double* hi, double* exp_avg, double* exp_avg_sq, double lr, double beta1, double beta2,
                             double eps, int64_t* steps_done, mobocmf_stream_t stream);

/* The k largest of vals (n), in descending order, ties to the lower index, NaN after every number: out_vals (k), out_idx (k,
 * int64) and, with x (n x d) given, the selected rows in out_x (k x d) (x and out_x both or neither; they must not overlap).
 * MOBOCMF_BAD_ARG: vals, out_vals or out_idx NULL; k outside 1..MOBOCMF_TOPK_MAX_K; n < k; n > MOBOCMF_TOPK_MAX_N; only one of
 * x / out_x given; with x, d outside 1..MOBOCMF_MAX_D. */
int mobocmf_select_topk(const double* vals, int32_t n, int32_t k, const double* x, int32_t d, double* out_vals,
                        int64_t* out_idx, double* out_x, mobocmf_stream_t stream);

/* ---- Predictive moments of fitted surrogates LARGER than the one-launch steps take (MOBOCMF_COOP_MAX_M < M <=
 * MOBOCMF_FROZEN_MAX_M) against their FROZEN chains, and the gradient w.r.t. the test points (csrc/frozen_predict.hip): the two
 * model evaluations of a device acquisition search at those sizes.  n models at the same kind of T test points; the parameters
 * are constants, so every layer's M x M chain exists already: chain[l] is the layer's CHAIN state, the first
 * `state_bytes` (mobocmf_chain_block_bytes) of the chain block mobocmf_layers_chain_forward with branch = 1 filled, read only.
 * The algebra is the layer's eval branch (no clamp, floor 1e-10), column by column:
 *   layer 0 at x_t:               k = k(Z, x_t), A = L^-1 k, C = U^T A, mean = a^T A, var = max(k_nn - |A|^2 + |C|^2, 1e-10)
 *   layer l >= 1 at column t S + s: f = mean_{l-1} + sqrt(var_{l-1}) samples[l][s] (layer 0's column t serves the S replicas),
 *                                 then the same with k = k([Z_x, zf_l], [x_t, f])
 * mode MOBOCMF_STEP_FORWARD: top_mean / top_var (T S; T for L = 1) <- the top layer's moments WITHOUT likelihood noise.
 * mode MOBOCMF_STEP_INPUT_GRADIENTS: the same, and grad (T x d) <- d / d x of <seed_gmean, top mean> + <seed_gvar, top var>
 *   (a column at the variance floor passes no variance gradient), summed over the layers and the S columns of a base row in a
 *   fixed order.  The launch forms its panels itself: it does not depend on an earlier FORWARD launch.
 * One launch on `stream`; a workgroup owns (model, a block of base rows) and nothing is shared between workgroups: no in-launch
 * wait, no atomics, no status word; two calls on the same inputs are bitwise equal; capturable (the FIRST call per device and
 * mode sets a function attribute and belongs outside a capture).  The kernel reads the descriptors from DEVICE memory
 * (dev_models); host_models is the same array in host memory, for validation and launch geometry.
 * Limits: 1 <= L <= MOBOCMF_TINY_MAX_LAYERS layers of kind 0, 1, 1 with one M; 1 <= M <= MOBOCMF_FROZEN_MAX_M (two [M][16]
 * panels in LDS); d <= MOBOCMF_TINY_MAX_D; L = 1: S = 1, else 2 <= S <= MOBOCMF_MAX_XDIV; T S <= MOBOCMF_ACQ_MAX_COLUMNS;
 * n_models <= 256.  MOBOCMF_BAD_ARG otherwise, for a NULL pointer among those the mode reads, or for another mode.
 * mobocmf_frozen_predict_work_bytes: the bytes of `work` a launch of `mode` needs -- 0 for both modes of this version (the
 * panels never leave LDS: a group built for values only, or for 5000 columns, holds no M x T S storage); work may then be NULL. */
#define MOBOCMF_FROZEN_MAX_M 512
typedef struct mobocmf_frozen_predict_model {
    int32_t L, M, d, S;
    int32_t T;                                   /* test points */
    int32_t kind[MOBOCMF_TINY_MAX_LAYERS];       /* 0, 1, 1 */
    const void* chain[MOBOCMF_TINY_MAX_LAYERS];  /* the layer's CHAIN state (state_bytes of mobocmf_chain_block_bytes) */
    const double* Zx[MOBOCMF_TINY_MAX_LAYERS];   /* M x d (the layers share one Z_x; the pointers may be equal) */
    const double* zf[MOBOCMF_TINY_MAX_LAYERS];   /* M (layers >= 1) */
    const double* hyp[MOBOCMF_TINY_MAX_LAYERS];  /* packed constrained hyper-parameters (the layer entry points' order) */
    const double* samples[MOBOCMF_TINY_MAX_LAYERS]; /* S (layers >= 1): the layer's fixed draws */
    const double* x;                             /* T x d, shared by the models of a group */
    double* top_mean;                            /* T S */
    double* top_var;
    const double* seed_gmean;                    /* T S (MOBOCMF_STEP_INPUT_GRADIENTS) */
    const double* seed_gvar;
    double* grad;                                /* T x d (MOBOCMF_STEP_INPUT_GRADIENTS) */
    void* work;                                  /* mobocmf_frozen_predict[_split]_work_bytes (NULL when that is 0) */
} mobocmf_frozen_predict_model;
int mobocmf_frozen_predict_work_bytes(const mobocmf_frozen_predict_model* model, int32_t mode, size_t* bytes);
int mobocmf_frozen_predict(const mobocmf_frozen_predict_model* host_models, const mobocmf_frozen_predict_model* dev_models,
                           int32_t n_models, int32_t mode, mobocmf_stream_t stream);

/* ---- The same for surrogates up to MOBOCMF_FROZEN_SPLIT_MAX_M inducing points: the same descriptors, modes, algebra and results
 * layout, on panels of 8 columns (two [M][8] panels and a: 136 KB of LDS at M = 1024) with the S replicas of a base row SPLIT over
 * workgroups.  L >= 2: a workgroup owns (model, base row t, part p) -- the replicas s in [8 p, 8 p + 8), ceil(S / 8) parts -- and
 * runs the whole chain for them (layer 0's column of row t is formed by every part); L = 1: a workgroup owns 8 base rows.
 * mode MOBOCMF_STEP_INPUT_GRADIENTS, L >= 2: every part writes its partial d / d x of its base row to `work` ([part][T][d]
 * doubles), and a second small kernel of the same call sums the parts in ascending order into grad; every slot it reads was
 * written by the first kernel of the same call.  L = 1 writes grad directly (no second kernel).  Nothing is shared between the
 * workgroups of a launch: no in-launch wait, no atomics, no status word; two calls on the same inputs are bitwise equal;
 * capturable (the FIRST call per device and mode sets a function attribute and belongs outside a capture).
 * mobocmf_frozen_predict_split_work_bytes: ceil(S / 8) T d 8 for MOBOCMF_STEP_INPUT_GRADIENTS with L >= 2, else 0.
 * Limits: those of mobocmf_frozen_predict with 1 <= M <= MOBOCMF_FROZEN_SPLIT_MAX_M; `work` non-NULL where its bytes are
 * non-zero.  MOBOCMF_BAD_ARG otherwise.  mobocmf_frozen_predict and its limit are unchanged by this entry point. */
#define MOBOCMF_FROZEN_SPLIT_MAX_M 1024
int mobocmf_frozen_predict_split_work_bytes(const mobocmf_frozen_predict_model* model, int32_t mode, size_t* bytes);
int mobocmf_frozen_predict_split(const mobocmf_frozen_predict_model* host_models, const mobocmf_frozen_predict_model* dev_models,
                                 int32_t n_models, int32_t mode, mobocmf_stream_t stream);

/* ---- Predictive moments of fitted EXACT-GP surrogates (the multi-fidelity baselines: two ARD-RBF kernels, a signal and a
 * noise one, combined by level factors) against a factorisation formed ONCE, and the gradient w.r.t. the test points
 * (csrc/exact_predict.hip): the two model evaluations of the MES baseline's device acquisition search.  n_models models at the
 * same T test points x; the models of a group may differ in n.  Linv and a are what mobocmf_exact_gp_factor leaves in its
 * state (L^-1, n x n lower with leading dimension ld, and a = L^-1 y), read only.  Per model and test point t:
 *   k_r  = sig[level] sig[lev_r] os_s exp(-1/2 sum_j ((x_tj - X_rj) / ls_s,j)^2)
 *        + ntab[min(level, lev_r)] os_n exp(-1/2 sum_j ((x_tj - X_rj) / ls_n,j)^2)                       r < n
 *   w    = Linv k      mean = a^T w      var = kss - |w|^2           (no clamp, no floor)
 * mode MOBOCMF_STEP_FORWARD: top_mean / top_var (T) <- the latent moments WITHOUT likelihood noise.
 * mode MOBOCMF_STEP_INPUT_GRADIENTS: the same, and with c = seed_gmean[t] a - 2 seed_gvar[t] w, e = Linv^T c:
 *   grad[t][j] = sum_r e_r dk_r/dx_tj,   dk_r/dx_tj = -(x_tj - X_rj) (signal term / ls_s,j^2 + noise term / ls_n,j^2),
 *   summed over r in ascending order.  The launch forms its panels itself: it does not depend on an earlier FORWARD launch.
 * One launch on `stream`; a workgroup owns (model, a block of 16 test points) and nothing is shared between workgroups: no
 * in-launch wait, no atomics, no status word; two calls on the same inputs are bitwise equal; capturable (the FIRST call per
 * device and mode sets a function attribute and belongs outside a capture).  Both triangular products run on
 * v_mfma_f64_16x16x4_f64 with the k and w panels ([n][16] each) in LDS.  The kernel reads the descriptors from DEVICE memory
 * (dev_models); host_models is the same array in host memory, for validation and launch geometry.  Rows beyond T and padded
 * training rows are never written.  The levels are device data: a lev_r outside [0, n_levels) makes that model's moments NaN
 * and is never used as an index.
 * Limits: 1 <= n <= MOBOCMF_EXACT_PREDICT_MAX_N (two 16-column panels are 128 KB of LDS); 1 <= d <= MOBOCMF_MAX_D; 1 <= T <=
 * MOBOCMF_TOPK_MAX_N; 1 <= n_levels <= MOBOCMF_EXACT_PREDICT_MAX_LEVELS; 0 <= level < n_levels; ld >= n; 1 <= n_models <=
 * 2 MOBOCMF_ACQ_MAX_PAIRS.  MOBOCMF_BAD_ARG otherwise, for a NULL pointer among those the mode reads, or for another mode -- on
 * the host, before any HIP call.
 * mobocmf_exact_predict_work_bytes: the bytes of `work` a launch of `mode` needs -- 0 for both modes of this version (the
 * panels never leave LDS); work may then be NULL. */
#define MOBOCMF_EXACT_PREDICT_MAX_N 512
#define MOBOCMF_EXACT_PREDICT_MAX_LEVELS 8
typedef struct mobocmf_exact_predict_model {
    int32_t n, d, T;                 /* training rows, input columns (without the fidelity column), test points */
    int32_t n_levels, level;         /* fidelity levels, and the level the test points are evaluated at */
    int32_t reserved;
    int64_t ld;                      /* leading dimension of Linv */
    const double* xtr;               /* n x d training inputs */
    const int32_t* lev;              /* n: their levels */
    const double* sig;               /* n_levels: signal factor per level (all ones for the min-level kernel) */
    const double* ntab;              /* n_levels: noise factor per min-level */
    const double* hyp_s;             /* 1 + d: [outputscale, lengthscale[0..d)] of the signal ARD-RBF */
    const double* hyp_n;             /* 1 + d: the noise ARD-RBF's */
    const double* Linv;              /* n x n lower, leading dimension ld */
    const double* a;                 /* n: L^-1 y */
    double kss;                      /* prior variance at `level`: sig[level]^2 os_s + ntab[level] os_n */
    const double* x;                 /* T x d, shared by the models of a group */
    double* top_mean;                /* T */
    double* top_var;
    const double* seed_gmean;        /* T (MOBOCMF_STEP_INPUT_GRADIENTS) */
    const double* seed_gvar;
    double* grad;                    /* T x d (MOBOCMF_STEP_INPUT_GRADIENTS) */
    void* work;                      /* mobocmf_exact_predict_work_bytes (NULL when that is 0) */
} mobocmf_exact_predict_model;
int mobocmf_exact_predict_work_bytes(const mobocmf_exact_predict_model* model, int32_t mode, size_t* bytes);
int mobocmf_exact_predict(const mobocmf_exact_predict_model* host_models, const mobocmf_exact_predict_model* dev_models,
                          int32_t n_models, int32_t mode, mobocmf_stream_t stream);

/* ---- Fitting the EXACT-GP surrogates on the device (csrc/exact_fit.hip): the launches of one Adam step on -log N(y | 0, K)
 * that are not the factorisation's, for n_models models at once (util/exact_fit.py: ExactGPFitStep captures the step once and
 * replays it).  Per model: x the n x d training inputs WITHOUT the fidelity column, lev their levels, and six parameter slots
 * (MOBOCMF_EXACT_FIT_P_*) each with its raw tensor and the constraint it carries: value = raw (IDENTITY), lo + softplus(raw)
 * (SOFTPLUS, torch's threshold 20), lo + (hi - lo) sigmoid(raw) (SIGMOID).  With tau, os_s, ls_s, os_n, ls_n, rho the values:
 *   E^k_ij = exp(-1/2 sum_c ((x_ic - x_jc) / ls_kc)^2)                                                  k in {s, n}
 *   K_ij   = sig[l_i] sig[l_j] os_s E^s_ij + ntab[min(l_i, l_j)] os_n E^n_ij + tau [i == j]
 *   KERNEL_MIN: sig = 1, ntab[t] = t.   KERNEL_LIN: sig[l] = prod_{q < l} rho_q,
 *                                       ntab[t] = [t >= 1] + sum_{k = 3}^{n_levels - 2} [t + 1 >= k] rho_{k-2}^2
 *   G = dmll / dK = (alpha alpha^T - K^-1) / 2,  alpha = L^-T a
 * mobocmf_exact_fit_covariance: K (n x n, tau on the diagonal) from the CURRENT raw parameters into the model's work area, ld
 *   npad = n rounded up to 128, zeros in the padding and identity on the padded diagonal: the input of mobocmf_exact_gp_factor,
 *   which the caller runs per model with mll / info / state where the descriptor says (Linv, a: inside that state).
 * mobocmf_exact_fit_prepare: LiT = Linv^T (npad x npad, the whole padded matrix) and alpha (npad, zero beyond n) into the work
 *   area.  The caller then forms Kinv = LiT LiT^T with mobocmf_gemm_f64 (tri = 2, trans_b = 1) into the work area.
 * mobocmf_exact_fit_gradient: a workgroup owns (model, strip of MOBOCMF_EXACT_FIT_STRIP rows i) and STORES, into row `strip`
 *   of the slab, its share of the MOBOCMF_EXACT_FIT_SUMS sums  sum_ij G_ij dK_ij / dvalue  -- G formed on the fly, both
 *   exponentials formed again -- in this order:
 *     [0] os_s   sum G sig_i sig_j E^s                     [1 + c] ls_s,c  sum G sig_i sig_j os_s E^s (x_ic - x_jc)^2 / ls_sc^3
 *     [33] os_n  sum G ntab[min] E^n                       [34 + c] ls_n,c the same with ntab[min] os_n E^n and ls_nc
 *     [66] tau   tr G       [67 + l] sig[l]  2 sum_{i: l_i = l} sum_j G sig_j os_s E^s       [75 + t] ntab[t]  sum_{min = t} G os_n E^n
 *   (entries of coordinates >= d are 0).  Wavefront shuffles, then LDS in wavefront order: no atomics.
 * mobocmf_exact_fit_update, MOBOCMF_EXACT_FIT_STEP, one workgroup per model, in this order: sums the slab strip by strip (also
 *   left in `sums` of the work area); reads loss = -mll[0] and info[0]; a stopped model (words[STOPPED_AT] >= 0): nothing; loss
 *   non-finite or info != 0: words[STOPPED_AT] = words[IT], losses[IT] = NaN, parameters untouched (info < 0, an abandoned
 *   in-launch wait of the factorisation, also sets the sticky words[ABANDONED]); else losses[IT] = loss, and if there is no best
 *   yet or loss < stats[0]: stats[0] = loss, words[BEST_IT] = IT, best <- raw (BEFORE the update); then the chain rule (through
 *   sig and ntab to rho by prefix and running products, no division; through the constraint's slope to raw; the sign of -mll)
 *   into grad, torch-default Adam on raw / exp_avg / exp_avg_sq with step count IT + 1 (the expressions of mobocmf_adam_multi),
 *   and words[IT] += 1.  MOBOCMF_EXACT_FIT_FINISH (after one more covariance + factorisation): stats[1] = the final loss,
 *   words[FINAL_INFO] = info; if a best exists and the final loss is non-finite, info != 0 or loss > stats[0]: raw <- best and
 *   words[RESTORED] = 1.  The caller initialises words (IT 0, STOPPED_AT -1, BEST_IT -1, the others 0), losses (NaN) and the
 *   Adam state (0).
 * Work area (doubles, mobocmf_exact_fit_work_bytes): K | LiT | Kinv (npad^2 each) | alpha (npad) | slab (ceil(n / 16) x 83) |
 * sums (83).  One launch each on `stream`, nothing shared between the workgroups of different models, no in-launch wait; two
 * runs are bitwise equal; capturable.  The kernels read the descriptors from DEVICE memory (dev_models); host_models is the
 * same array in host memory, for validation and launch geometry.  A level outside [0, n_levels) makes K and the sums NaN and is
 * never used as an index.
 * Limits: 1 <= n <= MOBOCMF_EXACT_FIT_MAX_N; 1 <= d <= MOBOCMF_MAX_D; 1 <= n_levels <= MOBOCMF_EXACT_FIT_MAX_LEVELS; 1 <=
 * n_models <= MOBOCMF_EXACT_FIT_MAX_MODELS; numel = 1 (noise, outputscales), d (lengthscales), n_levels - 1 (rho, KERNEL_LIN; 0
 * and no pointers for KERNEL_MIN); cap >= 1.  MOBOCMF_BAD_ARG otherwise, for a NULL pointer or for another mode, on the host
 * before any HIP call. */
#define MOBOCMF_EXACT_FIT_MAX_N 512
#define MOBOCMF_EXACT_FIT_MAX_LEVELS 8
#define MOBOCMF_EXACT_FIT_MAX_MODELS (2 * MOBOCMF_ACQ_MAX_PAIRS)
#define MOBOCMF_EXACT_FIT_STRIP 16
#define MOBOCMF_EXACT_FIT_SUMS (2 * (MOBOCMF_MAX_D + 1) + 1 + 2 * MOBOCMF_EXACT_FIT_MAX_LEVELS)
#define MOBOCMF_EXACT_FIT_KERNEL_MIN 0      /* MFKernel */
#define MOBOCMF_EXACT_FIT_KERNEL_LIN 1      /* MFKernel_lin */
#define MOBOCMF_EXACT_FIT_IDENTITY 0
#define MOBOCMF_EXACT_FIT_SOFTPLUS 1
#define MOBOCMF_EXACT_FIT_SIGMOID 2
#define MOBOCMF_EXACT_FIT_PARAMS 6
#define MOBOCMF_EXACT_FIT_P_NOISE 0
#define MOBOCMF_EXACT_FIT_P_OS_S 1
#define MOBOCMF_EXACT_FIT_P_LS_S 2
#define MOBOCMF_EXACT_FIT_P_OS_N 3
#define MOBOCMF_EXACT_FIT_P_LS_N 4
#define MOBOCMF_EXACT_FIT_P_RHO 5
#define MOBOCMF_EXACT_FIT_STEP 0
#define MOBOCMF_EXACT_FIT_FINISH 1
#define MOBOCMF_EXACT_FIT_WORDS 8
#define MOBOCMF_EXACT_FIT_W_IT 0
#define MOBOCMF_EXACT_FIT_W_STOPPED_AT 1
#define MOBOCMF_EXACT_FIT_W_BEST_IT 2
#define MOBOCMF_EXACT_FIT_W_RESTORED 3
#define MOBOCMF_EXACT_FIT_W_ABANDONED 4
#define MOBOCMF_EXACT_FIT_W_FINAL_INFO 5
typedef struct mobocmf_exact_fit_param {
    double* raw;                     /* the model's own parameter tensor, updated in place */
    double* best;                    /* the best iterate's copy */
    double* exp_avg;
    double* exp_avg_sq;
    double* grad;                    /* d(-mll) / d raw of the last step */
    int32_t numel, kind;             /* MOBOCMF_EXACT_FIT_IDENTITY / SOFTPLUS / SIGMOID */
    double lo, hi;
} mobocmf_exact_fit_param;
typedef struct mobocmf_exact_fit_model {
    int32_t n, d, n_levels, kernel;  /* training rows, input columns, fidelity levels, MOBOCMF_EXACT_FIT_KERNEL_* */
    int32_t cap, reserved;           /* entries of losses */
    const double* x;                 /* n x d */
    const int32_t* lev;              /* n */
    const double* y;                 /* n (what the caller hands to mobocmf_exact_gp_factor) */
    mobocmf_exact_fit_param params[MOBOCMF_EXACT_FIT_PARAMS];
    const double* Linv;              /* npad x npad and npad, inside the factorisation's state */
    const double* a;
    const double* mll;               /* the factorisation's likelihood and info words */
    const int32_t* info;
    double* losses;                  /* cap */
    double* stats;                   /* 2: best loss, final loss */
    int32_t* words;                  /* MOBOCMF_EXACT_FIT_WORDS */
    void* work;                      /* mobocmf_exact_fit_work_bytes */
} mobocmf_exact_fit_model;
int mobocmf_exact_fit_work_bytes(const mobocmf_exact_fit_model* model, int32_t n_models, size_t* bytes);
int mobocmf_exact_fit_covariance(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                                 int32_t n_models, mobocmf_stream_t stream);
int mobocmf_exact_fit_prepare(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                              int32_t n_models, mobocmf_stream_t stream);
int mobocmf_exact_fit_gradient(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                               int32_t n_models, mobocmf_stream_t stream);
int mobocmf_exact_fit_update(const mobocmf_exact_fit_model* host_models, const mobocmf_exact_fit_model* dev_models,
                             int32_t n_models, int32_t mode, double lr, double beta1, double beta2, double eps,
                             mobocmf_stream_t stream);

/* ---- Posterior FUNCTION samples of the EXACT-GP surrogates on the device (csrc/exact_sample.hip): the stage of a max-value
 * entropy search iteration between the fit and the acquisition search, for n_problems (model, sample) problems of different n
 * at once (util/exact_sample.py).  Both baseline kernels have the form
 *   k([x, t], [x', t']) = s(t) s(t') k_sig(x, x') + ntab[min(t, t')] k_noi(x, x'),     ntab[m] = sum_{l <= m} delta_l, delta_l >= 0
 * (sig / ntab: the tables of mobocmf_exact_predict; sqd[l] = sqrt(delta_l)).  With F random features per ARD-RBF kernel,
 *   C_sig = cos(W_sig x + b_sig),  C_noi = cos(W_noi x + b_noi)   (F x n; W already divided by the lengthscales)
 *   c_sig = sqrt(2 a_sig / F),     c_noi = sqrt(2 a_noi / F)      (scal = [a_sig, a_noi, noise], device data)
 * the weight-space feature map Phi has (1 + n_levels) F rows: block 0 is s(l_i) c_sig C_sig[:, i]; block 1 + l is
 * sqd[l] c_noi C_noi[:, i] for the rows with l_i >= l and zero for the others.  Matheron's rule in the n-dimensional function
 * space, theta0 ~ N(0, I) ((1 + n_levels) F, block order) and e ~ N(0, noise I_n) being OPERANDS (the kernels draw nothing):
 *   G     = Phi^T Phi + noise I
 *         = s_i s_j c_sig^2 (C_sig^T C_sig)_ij + ntab[min(l_i, l_j)] c_noi^2 (C_noi^T C_noi)_ij + noise [i == j]
 *   r     = y - Phi^T theta0 - e
 *   w     = G^-1 r
 *   theta = theta0 + Phi w
 * and the sampled function at output level f is ONE random-feature layer of 2F features,
 *   g_f(x) = s(f) c_sig theta_sig . cos(W_sig x + b_sig) + c_noi (sum_{l <= f} sqd[l] theta_noi,l) . cos(W_noi x + b_noi).
 * mobocmf_exact_sample_gram: G of every problem in one launch, ld npad = n rounded up to 128, zeros in the padding and identity
 *   on the padded diagonal (the input of mobocmf_exact_gp_factor, as mobocmf_exact_fit_covariance writes it), and r (n).  A
 *   workgroup owns a 64 x 64 tile on or below the diagonal and stores its mirror image too; the cosines are formed in LDS in
 *   chunks of MOBOCMF_EXACT_SAMPLE_CHUNK features and both n x n x F products run on v_mfma_f64_16x16x4_f64 from there: Phi is
 *   never written to memory; the level and scale combination is the epilogue.
 * The caller then runs mobocmf_exact_gp_factor per problem with r as its right-hand side (Linv, a, info: where the descriptor
 *   says).
 * mobocmf_exact_sample_weights: two launches -- w = L^-T a (n) and info_out[0] = info[0]; then theta ((1 + n_levels) F, block
 *   order) and, for each of the n_out requested levels out_level[o], the packed one-layer chain sample (layers/rff.py,
 *   RFFChainSample.pack: header 1, 1, d, 2F, length, kind 0; alpha = F, 0, 0, 0, s0 = 1, 0, 0; W1 = [W_sig; W_noi] (2F x d);
 *   b1 = [b_sig; b_noi]; theta' = [s(f) c_sig theta_sig; c_noi sum_{l <= f} sqd[l] theta_noi,l]) at chain + o (13 + 2F (d + 2)).
 * Nothing is shared between workgroups, sums run in a fixed order: no atomics, no in-launch wait; two runs are bitwise equal.
 * The kernels read the descriptors from DEVICE memory (dev_problems); host_problems is the same array in host memory, for
 * validation and launch geometry.  A level outside [0, n_levels) makes G, r and theta NaN and is never used as an index.
 * Limits: 1 <= n <= MOBOCMF_EXACT_SAMPLE_MAX_N; 1 <= d <= MOBOCMF_MAX_D; 1 <= n_levels <= MOBOCMF_EXACT_SAMPLE_MAX_LEVELS;
 * 1 <= F <= MOBOCMF_EXACT_SAMPLE_MAX_F; 0 <= n_out <= MOBOCMF_EXACT_SAMPLE_MAX_LEVELS, 0 <= out_level[o] < n_levels; 1 <=
 * n_problems <= MOBOCMF_EXACT_SAMPLE_MAX_PROBLEMS.  MOBOCMF_BAD_ARG otherwise or for a NULL pointer among those the entry point
 * uses, on the host before any HIP call. */
#define MOBOCMF_EXACT_SAMPLE_MAX_N 512
#define MOBOCMF_EXACT_SAMPLE_MAX_LEVELS 8
#define MOBOCMF_EXACT_SAMPLE_MAX_F 65536
#define MOBOCMF_EXACT_SAMPLE_MAX_PROBLEMS (2 * MOBOCMF_ACQ_MAX_PAIRS)
#define MOBOCMF_EXACT_SAMPLE_CHUNK 16
typedef struct mobocmf_exact_sample_problem {
    int32_t n, d, n_levels, F;       /* training rows, input columns (without the fidelity column), levels, features per kernel */
    int32_t n_out, reserved;         /* output levels of the weights launch */
    int32_t out_level[MOBOCMF_EXACT_SAMPLE_MAX_LEVELS];
    const double* x;                 /* n x d */
    const int32_t* lev;              /* n */
    const double* y;                 /* n */
    const double* sig;               /* n_levels: s(level) */
    const double* ntab;              /* n_levels */
    const double* sqd;               /* n_levels: sqrt(ntab[l] - ntab[l - 1]), sqrt(ntab[0]) */
    const double* scal;              /* 3: a_sig, a_noi, noise */
    const double* W_sig;             /* F x d */
    const double* b_sig;             /* F */
    const double* W_noi;
    const double* b_noi;
    const double* theta0;            /* (1 + n_levels) F */
    const double* e;                 /* n */
    double* G;                       /* npad x npad (gram) */
    double* r;                       /* n (gram) */
    const double* Linv;              /* npad x npad and npad, inside the factorisation's state (weights) */
    const double* a;
    const int32_t* info;             /* the factorisation's info word */
    double* w;                       /* n */
    double* theta;                   /* (1 + n_levels) F */
    double* chain;                   /* n_out x (13 + 2F (d + 2)) */
    int32_t* info_out;
} mobocmf_exact_sample_problem;
int mobocmf_exact_sample_gram(const mobocmf_exact_sample_problem* host_problems, const mobocmf_exact_sample_problem* dev_problems,
                              int32_t n_problems, mobocmf_stream_t stream);
int mobocmf_exact_sample_weights(const mobocmf_exact_sample_problem* host_problems, const mobocmf_exact_sample_problem* dev_problems,
                                 int32_t n_problems, mobocmf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOBOCMF_HIP_H */
