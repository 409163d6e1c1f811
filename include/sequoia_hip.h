/* libsequoia_hip.so -- C ABI of the MI355X-native SEQUOIA hot path.
 *
 * The reference (gevaertlab/sequoia-pub) has no FFI / plugin interface: the path is
 * reached through three Python object interfaces.  Each entry
 * point below states the reference interface it stands behind (file:line under
 * /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: every function returns 0 on success and a negative code on error
 * (message: sq_last_error(), thread-local).  Nothing here allocates device memory:
 * the caller (PyTorch-ROCm is only the allocator) passes raw device pointers,
 * element counts and a workspace whose size is queried with *_workspace_bytes.
 * Every call is asynchronous on the given hipStream_t.  Plain C types only.
 */
#ifndef SEQUOIA_HIP_H
#define SEQUOIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sq_stream_t; /* hipStream_t */
typedef void* sq_event_t;  /* hipEvent_t */

#define SQ_OK 0
#define SQ_ERR_ARG -1         /* an argument is outside what the entry admits; nothing was launched */
#define SQ_ERR_HIP -2         /* a HIP runtime call failed */
#define SQ_ERR_WORKSPACE -3   /* the workspace is smaller than *_workspace_bytes says */
#define SQ_ERR_UNSUPPORTED -4 /* well-formed arguments the entry cannot serve (sq_resize_u8, sq_emd_status_check) */

#define SQ_DTYPE_F32 0  /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): parity mode */
#define SQ_DTYPE_BF16 1 /* bf16 MFMA, fp32 accumulate: perf mode              */
#define SQ_DTYPE_BF16X3 2 /* split bf16 (sq_resnet50_extract only): every fp32 value as hi + lo bf16 planes, a.b = a_hi.b_hi + a_hi.b_lo +
                             a_lo.b_hi on bf16 MFMAs with fp32 accumulation -- 2^-18 per operand, fp32's exponent range */
#define SQ_DTYPE_F16X3 3  /* the same with fp16 planes: 22 significant bits (fp32-class results), values must stay below 65504
                             (an overflow propagates to the features as NaN and raises sq_resnet50_extract_checked's flag); the fast parity mode */

#define SQ_MAX_DEPTH 16
#define SQ_HEAD_DIM 64 /* dimensions_f = dimensions_s = dimensions_c = 64 (src/main.py:147,167,202) */

const char* sq_last_error(void);
int sq_version(void);
/* 1 when a gfx950 device is visible to the HIP runtime, else 0 (never fails) */
int sq_device_ok(void);

/* HIP-event timing of the library's own launches (bench.py roofline leg; no reference
 * counterpart).  sq_prof_enable(1) makes every instrumented launch record two events on
 * its stream; sq_prof_report writes a JSON array of {name,count,total_ms,flops,bytes}
 * (flops/bytes = algorithmic work per launch) into buf and clears the records.
 * sq_prof_enable(2) additionally brackets every instrumented launch with marker launches whose grid size
 * carries the launch's class number ((id + 2) blocks of 64 threads in front, one block behind), so that a
 * dispatch-ordered counter trace (rocprofv3 --kernel-trace --pmc) can be attributed to classes without
 * knowing kernel symbols; sq_prof_marker_names writes the JSON array id -> class name. */
int sq_prof_enable(int on);
int sq_prof_report(char* buf, size_t cap);
int sq_prof_marker_names(char* buf, size_t cap);

/* ------------------------------------------------------------------------------
 * ViS aggregator  (src/tformer_lin.py:80-106 ViS; :64-77 SummaryTransformer;
 * :29-48 MultiHeadSummary; :7-26 SummaryMixing; :51-61 FeedForward)
 * ---------------------------------------------------------------------------- */
typedef struct sq_vis_config {
    int32_t input_dim;    /* D: 1024 (UNI) or 2048 (ResNet-50); multiple of 64 */
    int32_t depth;        /* main.py:36 default 6 */
    int32_t nheads;       /* main.py:37 default 16 */
    int32_t num_outputs;  /* G = 20820 genes */
    int32_t num_clusters; /* 100 tokens (tformer_lin.py:83) */
} sq_vis_config;

/* Offsets (in elements) of every reference tensor inside ONE flat parameter buffer.
 * Per-head tensors are stored head-major and contiguous, so each reference tensor
 * `transformer.layers.{l}.0.mixers.{h}.f.weight` etc. is a contiguous slice. */
typedef struct sq_vis_layer_offsets {
    int64_t f_w, f_b;       /* mixers.{h}.f.{weight,bias}              [H][64][D], [H][64] */
    int64_t s_w, s_b;       /* mixers.{h}.s.{weight,bias}              [H][64][D], [H][64] */
    int64_t lnf_g, lnf_b;   /* mixers.{h}.local_norm.{weight,bias}     [H][64]             */
    int64_t lns_g, lns_b;   /* mixers.{h}.summary_norm.{weight,bias}   [H][64]             */
    int64_t c_w, c_b;       /* mixers.{h}.c.{weight,bias}              [H][64][128], [H][64] */
    int64_t proj_w, proj_b; /* projection.{weight,bias}                [D][H*64], [D]      */
    int64_t ffln_g, ffln_b; /* net.0 LayerNorm(D)                                           */
    int64_t ff1_w, ff1_b;   /* net.1 Linear(D, D)                                           */
    int64_t ff2_w, ff2_b;   /* net.3 Linear(D, D)                                           */
} sq_vis_layer_offsets;

typedef struct sq_vis_layout {
    int64_t pos;                  /* pos_emb1D [num_clusters][D] */
    int64_t head_ln_g, head_ln_b; /* linear_head.0 */
    int64_t head_w, head_b;       /* linear_head.1 [G][D], [G] */
    int64_t total;                /* elements in the flat buffer */
    sq_vis_layer_offsets layer[SQ_MAX_DEPTH];
} sq_vis_layout;

int sq_vis_layout_init(const sq_vis_config* cfg, sq_vis_layout* out);

size_t sq_vis_workspace_bytes(const sq_vis_config* cfg, int dtype, int batch, int save_for_backward);

/* ViS.forward (tformer_lin.py:97-106): x f32 [B, num_clusters, D] -> out f32 [B, G].
 * params: flat fp32 buffer (sq_vis_layout); params_lp: bf16 copy of the same buffer
 * (dtype == SQ_DTYPE_BF16) or NULL.  save_for_backward keeps the per-layer activations
 * sq_vis_backward needs in the workspace. */
int sq_vis_forward(const sq_vis_config* cfg, int dtype, const float* params, const void* params_lp, const float* x,
                   float* out, int batch, int save_for_backward, void* workspace, size_t workspace_bytes,
                   sq_stream_t stream);

/* sq_vis_forward with two options the sliding-window path (spatial_vis/visualize.py:35-102) uses:
 *  - gather: instead of x, give gather_src f32 [gather_rows, D] (the tile-feature cache) and gather_idx int32
 *    [B, num_clusters]; token (b, t) is row gather_idx[b, t] of the cache, a negative index is a zero row (the
 *    zero padding of visualize.py:72-75) -- the [B, 100, D] window batch is never materialised;
 *  - head_in: instead of out, receive the linear head's INPUT LayerNorm(mean_tokens X) as f32 [B, D]; the head is
 *    linear, so the per-tile mean over windows (visualize.py:97-100) can be taken on these D-vectors and the head
 *    applied once per tile (sq_linear) instead of materialising [n_windows, G] predictions.
 * Exactly one of (x | gather_src + gather_idx) and exactly one of (out | head_in) must be given. */
int sq_vis_forward_ex(const sq_vis_config* cfg, int dtype, const float* params, const void* params_lp, const float* x,
                      const float* gather_src, const int32_t* gather_idx, int gather_rows, float* out, float* head_in,
                      int batch, int save_for_backward, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* The gather + head_in form of sq_vis_forward_ex for the window loop of spatial_vis/visualize.py:46-82, with the first layer's
 * local projection f (src/tformer_lin.py:20, mixers.{h}.f of layer 0, all heads) taken from per-TILE projections: f is linear in
 * x = tile feature + pos_emb1D (tformer_lin.py:99-100), so for token (b, t)  f(x) = f_tile[gather_idx[b, t]] + f_pos[t]  with
 *   f_tile f32 [gather_rows, nheads*64] = cache . Wf^T            (no bias; a negative index contributes a zero row)
 *   f_pos  f32 [num_clusters, nheads*64] = pos_emb1D . Wf^T + bf
 * computed by the caller once per slide (two sq_linear calls) instead of once per window token.  Inference only. */
int sq_vis_forward_tiles(const sq_vis_config* cfg, int dtype, const float* params, const void* params_lp, const float* gather_src,
                         const int32_t* gather_idx, int gather_rows, const float* f_tile, const float* f_pos, float* head_in,
                         int batch, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* Backward of ViS.forward -- replaces torch autograd over tformer_lin.py in the training loop
 * (src/vit.py:163-180 `loss.backward()`).  grad_out f32 [B, G]; grad_params: flat f32 buffer with
 * the parameter layout, fully overwritten; grad_x f32 [B, num_clusters, D] or NULL.
 * fwd_workspace must be the workspace of the matching sq_vis_forward(save_for_backward = 1).
 * Training needs nheads to be a power of two (1, 2, 4, ..., 64); the forward pass takes any nheads in 1..64.  Another nheads is
 * refused with SQ_ERR_ARG before anything is launched (sq_vis_backward_workspace_bytes returns 0 and sets the same message). */
size_t sq_vis_backward_workspace_bytes(const sq_vis_config* cfg, int dtype, int batch);
int sq_vis_backward(const sq_vis_config* cfg, int dtype, const float* params, const void* params_lp,
                    const float* grad_out, float* grad_params, float* grad_x, int batch, void* fwd_workspace,
                    size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, sq_stream_t stream);

/* Data-parallel training (src/main.py DDP-less reference; BASELINE config 4): the flat gradient splits into
 * depth + 1 contiguous buckets [lo, hi) (elements), listed in the order the backward pass finishes them (head
 * first, then layers last to first; layer 0's bucket also holds pos_emb1D).  sq_vis_backward_buckets records
 * bucket_events[i] (hipEvent_t) on `stream` as soon as bucket i is final, so the caller can start that bucket's
 * RCCL all-reduce on another stream while the rest of the backward pass still runs.  Returns the bucket count. */
int sq_vis_grad_buckets(const sq_vis_config* cfg, int64_t* lo, int64_t* hi, int cap);
int sq_vis_backward_buckets(const sq_vis_config* cfg, int dtype, const float* params, const void* params_lp,
                            const float* grad_out, float* grad_params, float* grad_x, int batch, void* fwd_workspace,
                            size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, sq_stream_t stream,
                            const sq_event_t* bucket_events, int n_bucket_events);


/* ------------------------------------------------------------------------------
 * Softmax ViT baseline  (src/vit.py:49-115: Attention :49-74, Transformer :76-89, ViT :91-115;
 * `--model_type vit`, src/main.py:160-163: mlp_dim 2048, dim_head 64).  Same conventions as ViS:
 * one flat fp32 parameter buffer (sq_vit_layout), optional bf16 shadow, workspace from *_workspace_bytes.
 * ---------------------------------------------------------------------------- */
typedef struct sq_vit_config {
    int32_t dim, depth, heads, mlp_dim, num_outputs, num_clusters; /* dim_head = 64 */
} sq_vit_config;
typedef struct sq_vit_layer_offsets {
    int64_t ln1_g, ln1_b; /* layers.{l}.0.norm                         */
    int64_t qkv_w;        /* layers.{l}.0.to_qkv.weight [3*heads*64][dim] */
    int64_t out_w;        /* layers.{l}.0.to_out.weight [dim][heads*64]   */
    int64_t ln2_g, ln2_b; /* layers.{l}.1.net.0                         */
    int64_t ff1_w, ff1_b; /* layers.{l}.1.net.1 Linear(dim, mlp_dim)    */
    int64_t ff2_w, ff2_b; /* layers.{l}.1.net.3 Linear(mlp_dim, dim)    */
} sq_vit_layer_offsets;
typedef struct sq_vit_layout {
    int64_t pos, head_ln_g, head_ln_b, head_w, head_b, total;
    sq_vit_layer_offsets layer[SQ_MAX_DEPTH];
} sq_vit_layout;
int sq_vit_layout_init(const sq_vit_config* cfg, sq_vit_layout* out);
size_t sq_vit_workspace_bytes(const sq_vit_config* cfg, int dtype, int batch, int save_for_backward);
int sq_vit_forward(const sq_vit_config* cfg, int dtype, const float* params, const void* params_lp, const float* x,
                   float* out, int batch, int save_for_backward, void* workspace, size_t workspace_bytes,
                   sq_stream_t stream);
/* sq_vit_forward with the two options of sq_vis_forward_ex, for the window loop of spatial_vis/visualize.py:46-82 with
 * --model_type vit (the model: src/vit.py:105-115):
 *  - gather: instead of x, give gather_src f32 [gather_rows, D] (the tile-feature cache) and gather_idx int32 [B, num_clusters];
 *    token (b, t) is row gather_idx[b, t] of the cache plus pos_emb1D[t] (vit.py:109).  An index outside [0, gather_rows) -- a
 *    negative one in particular -- is a zero row (the zero padding of visualize.py:72-75); the window batch is never materialised;
 *  - head_in: instead of out, receive the linear head's INPUT LayerNorm(mean_tokens X) (vit.py:113-115) as f32 [B, D] in both
 *    dtypes; the [B, G] head product is skipped (the head is linear: the caller votes these vectors per tile, then applies it).
 * Exactly one of (x | gather_src + gather_idx) and exactly one of (out | head_in) must be given. */
int sq_vit_forward_ex(const sq_vit_config* cfg, int dtype, const float* params, const void* params_lp, const float* x,
                      const float* gather_src, const int32_t* gather_idx, int gather_rows, float* out, float* head_in,
                      int batch, int save_for_backward, void* workspace, size_t workspace_bytes, sq_stream_t stream);
/* Backward of sq_vit_forward(save_for_backward = 1).  The attention backward kernel keeps one (slide, head) in LDS --
 * 4 * (257 N + N^2) bytes of the 160 KiB -- so it needs num_clusters <= 111; the forward pass takes num_clusters up to 128.
 * 112..128 are refused with SQ_ERR_ARG before anything is launched. */
size_t sq_vit_backward_workspace_bytes(const sq_vit_config* cfg, int dtype, int batch);
int sq_vit_backward(const sq_vit_config* cfg, int dtype, const float* params, const void* params_lp,
                    const float* grad_out, float* grad_params, float* grad_x, int batch, void* fwd_workspace,
                    size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------
 * Training-step pieces of src/vit.py:117-243 `train`
 * ---------------------------------------------------------------------------- */
/* Scratch contract: a device buffer of sq_train_scratch_bytes(num_outputs) bytes, 8-byte aligned, serves sq_mse_loss_grad for
 * any n and sq_batch_metrics for that num_outputs (any batch); neither writes a byte beyond it.  Contents on entry are
 * ignored, contents on return unspecified; calls sharing one scratch must be ordered on one stream.
 * Alignment of the data pointers of the three entries below: natural (4 bytes for float, 2 for the bf16 shadow) -- the
 * kernels are element-wise, so any element range of a flat buffer may be passed. */
size_t sq_train_scratch_bytes(int num_outputs);
/* nn.MSELoss() (vit.py:129,166): *loss_out = mean((pred-target)^2) over n elements (device scalar);
 * grad[i] = grad_scale * (pred[i]-target[i])  (grad_scale = 2/n for the plain loss; grad may be NULL: the loss is the
 * same bits).  The difference is taken in fp32, its squares are summed in fp64 in a fixed order and rounded to float once.
 * n == 0 or a null pred / target / loss_out / scratch: SQ_ERR_ARG, nothing launched. */
int sq_mse_loss_grad(const float* pred, const float* target, size_t n, float grad_scale, float* grad, float* loss_out,
                     void* scratch, sq_stream_t stream);
/* torch.optim.AdamW(lr, amsgrad=False, weight_decay) (src/main.py:180-183) on a flat fp32 buffer;
 * step is the 1-based step count; grads are multiplied by grad_scale first (1/world for an
 * all-reduced sum); params_lp (bf16 shadow) is refreshed in the same pass when not NULL: round-to-nearest-even of the
 * parameters this call wrote; with NULL params / exp_avg / exp_avg_sq come out the same bits.  Every element is updated
 * on its own, so one call over [0, n) equals calls over any partition of it into slices, bit for bit (SQ_ADAMW_BUCKETS).
 * Hyperparameter precision: the ABI passes float.  1 - beta and beta^step are formed from those floats (torch forms them
 * from the Python doubles), so with beta2 = 0.999 the second moment sits about 1.3e-5 relative below torch's; the effect on
 * a parameter is below one fp32 rounding of the update (tests/train_prim_cases.py measures both).
 * n == 0, step < 1 or a null params / grads / exp_avg / exp_avg_sq: SQ_ERR_ARG, nothing launched. */
int sq_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* params_lp, size_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                  sq_stream_t stream);
/* Per-batch metrics the reference computes on the host every batch (vit.py:167-168):
 * out3[0] = sklearn mean_absolute_error, out3[1] = compute_correlations (src/he2rna.py:140-149:
 * mean per-gene Pearson r over genes with a non-constant target, NaN r dropped), out3[2] = #genes used.
 * With no gene used (batch == 1 in particular) out3[1] is NaN, as np.mean([]), and out3[2] is 0; out3[0] is still the MAE.
 * scratch: sq_train_scratch_bytes(num_outputs) bytes.  batch < 1, num_outputs < 1 or a null pointer: SQ_ERR_ARG. */
int sq_batch_metrics(const float* pred, const float* target, int batch, int num_outputs, float* out3, void* scratch,
                     sq_stream_t stream);

/* Per-gene test-set statistics of evaluation/evaluate_model.py:67-96 for real / pred / random [n, G] (row-major,
 * n = test slides <= 8192).  out9 is double [9][G]: 0 r(real, pred), 1 r(real, random), 2 r(pred, random)
 * (scipy.stats.pearsonr: centred, clipped to [-1, 1]; NaN when a column is constant), 3 RMSE(real, pred),
 * 4 RMSE(real, random), 5 mean(real), 6 / 7 the 0.25 / 0.75 quantiles of real (numpy linear method),
 * 8 = 1.0 when any of the three columns is constant (the reference's len(set(col)) == 1 branch).
 * The p-values (Student t, Steiger) are O(G) host arithmetic on these. */
size_t sq_gene_eval_workspace_bytes(int n, int num_outputs);
int sq_gene_eval_stats(const float* real, const float* pred, const float* random_pred, int n, int num_outputs, double* out9,
                       void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* Per-tile vote of sliding-window predictions (spatial_vis/visualize.py:86-101): win_pred f32 [n_windows, G];
 * tile_windows int32 [n_tiles, max_votes] = the windows containing each tile in visiting order, packed, -1 padded.
 * mode 0: out[t] = mean of the listed rows (stride < 10, :97-101); mode 1: the last listed row (stride 10: later
 * windows overwrite, :90-92).  Tiles in no kept window get `fill`.  out f32 [n_tiles, G]. */
int sq_window_vote(const float* win_pred, int n_windows, int num_outputs, const int32_t* tile_windows, int n_tiles,
                   int max_votes, int mode, float fill, float* out, sq_stream_t stream);

/* ------------------------------------------------------------------------------
 * Per-slide k-Means + cluster means  (pre_processing/kmean_features.py:96-108:
 *   KMeans(n_clusters=100, random_state=0).fit(features).labels_ ; per-label np.mean(...))
 * scikit-learn semantics (k-means++ with 2+log(k) local trials, Lloyd, max_iter 300, tol 1e-4),
 * batched over n_slides independent slides of n_samples x dim fp32 features each.
 * The MT19937 draws are data-independent, so the host passes them in: first_center =
 * RandomState(0).choice(n) and uniforms f64 [n_clusters-1, n_local_trials] (device memory).
 * Outputs (device): labels i32 [S, n]; cluster_features f32 [S, k, dim] (may be NULL);
 * seed_indices i32 [S, k] (may be NULL); n_iter i32 [S] (may be NULL).
 * Synchronises the stream between Lloyd bursts (the stop decision is read on the host).
 * max_iter is any int and tol any double.  max_iter <= 0 runs no Lloyd iteration: n_iter = 0, the centres stay the seeded
 * rows and labels are the one E-step against them (what scikit-learn's loop does when it is not entered); cluster_features
 * follow those labels.  tol is relative (scikit-learn's tol): the loop stops once the squared centre shift of an iteration
 * is <= tol * mean(var(X, axis=0)); tol = 0 leaves the label rule and max_iter.
 * The three entries below share one driver and one set of kernels: a call's slides lie back to back and a slide table
 * in the workspace says where each starts.  They differ in how that table is filled -- n_slides equal slides, one slide
 * of up to 65536 patches, or slides of different patch counts -- and in their bounds.  Common to all: n_clusters <= 256,
 * dim a multiple of 4, 1 <= n_local_trials <= 8; the sizes are checked before the device pointers and anything refused
 * leaves an sq_last_error message that names the bound; a short workspace gives SQ_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------- */
size_t sq_kmeans_workspace_bytes(int n_slides, int n_samples, int dim, int n_clusters);
int sq_kmeans_fit(const float* X, int n_slides, int n_samples, int dim, int n_clusters, int first_center,
                  const double* uniforms, int n_local_trials, int max_iter, double tol, int32_t* labels,
                  float* cluster_features, int32_t* seed_indices, int32_t* n_iter, void* workspace,
                  size_t workspace_bytes, sq_stream_t stream);

/* The same fit for ONE slide of any size up to SQ_KMEANS_LARGE_MAX_SAMPLES = 65536 patches (kmean_features.py:96-108 on
 * a slide made with a raised --max_patch_number, compute_features_hdf5.py:26,112-113; sq_kmeans_fit stops at 4096).
 * Same arithmetic, arguments and outputs as sq_kmeans_fit with n_slides = 1; the k-means++ seeding forms only the
 * distances of a step's candidates (no n x n Gram matrix) and the member lists come from a chunked counting sort.
 * Valid for every n_clusters <= n_samples <= 65536 (small slides included).
 * sq_kmeans_large_workspace_bytes returns 0 when n_samples is outside [1, 65536] (or dim / n_clusters < 1).
 * Synchronises the stream between Lloyd bursts (the stop decision is read on the host); the seeding adds no
 * synchronisation. */
#define SQ_KMEANS_LARGE_MAX_SAMPLES 65536
size_t sq_kmeans_large_workspace_bytes(int n_samples, int dim, int n_clusters);
int sq_kmeans_fit_large(const float* X, int n_samples, int dim, int n_clusters, int first_center, const double* uniforms,
                        int n_local_trials, int max_iter, double tol, int32_t* labels, float* cluster_features,
                        int32_t* seed_indices, int32_t* n_iter, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* The same fit for n_slides slides of DIFFERENT patch counts in one call: what the loop over slides of
 * kmean_features.py:65-108 computes, one fit per slide, for a whole group of them (compute_features_hdf5.py writes however
 * many patches passed the tissue filter, so the slides of a cohort never share a count and sq_kmeans_fit cannot batch them).
 * X f32 [sum n_samples, dim] holds the slides' rows back to back in list order, labels i32 [sum n_samples] likewise;
 * cluster_features f32 [S, k, dim], seed_indices i32 [S, k], n_iter i32 [S] (each may be NULL).
 * n_samples and first_centers are HOST arrays [S] (first_centers[s] = RandomState(seed).choice(n_samples[s])); uniforms is
 * the ONE device table f64 [n_clusters-1, n_local_trials] -- the MT19937 uniforms do not depend on the patch count.  The
 * entry copies the host arrays into its slide table before it returns: both may be reused or freed as soon as the call
 * returns.
 * Contract: for every slide, labels, seed_indices, n_iter and cluster_features are bit-equal to those of sq_kmeans_fit
 * (n_slides = 1) on that slide alone, whatever the other slides of the call are and wherever it sits in the list (the
 * seeding kernel's layout follows each slide's own n_samples; no padding rows exist).
 * Valid for 1 <= n_slides <= 4096, n_clusters <= n_samples[s] <= 4096 and 0 <= first_centers[s] < n_samples[s] for every
 * slide; a caller can ask with NULL data why a shape is refused.  sq_kmeans_ragged_workspace_bytes returns 0 for a shape
 * the entry refuses.  Synchronises the stream between Lloyd bursts, once for all slides of the call. */
size_t sq_kmeans_ragged_workspace_bytes(int n_slides, const int32_t* n_samples /*host [S]*/, int dim, int n_clusters);
int sq_kmeans_fit_ragged(const float* X, int n_slides, const int32_t* n_samples /*host [S]*/, int dim, int n_clusters,
                         const int32_t* first_centers /*host [S]*/, const double* uniforms, int n_local_trials, int max_iter,
                         double tol, int32_t* labels, float* cluster_features, int32_t* seed_indices, int32_t* n_iter,
                         void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------
 * ResNet-50 patch embedding (src/resnet.py:155-170 forward_extract; :73-93 Bottleneck;
 * :98-136 topology; eval-mode BN; patch transform pre_processing/compute_features_hdf5.py:49-51,119-120)
 * Weights are packed by the caller per sq_resnet50_layout: conv i at w_off (elements) as
 * [cout][kh][kw][cin] (conv 0: K = 147 zero-padded to k_padded = 152) with eval-mode BatchNorm
 * folded in, bias (fp32) at b_off.  Conv order: conv1; then per bottleneck conv1, conv2, conv3,
 * [downsample.0 for the first block of each layer].
 * dtype SQ_DTYPE_BF16X3 / SQ_DTYPE_F16X3: `weights` = the 16-bit hi plane [w_total] followed by the lo plane [w_total]
 * (hi = cvt(w'), lo = cvt(w' - hi)) of the packed fp32 weights w' = w * s[cout], and `bias` = [b_total] biases followed by
 * [b_total] per-output-channel factors 1 / s (at the same b_off): s = 1 for bf16 planes; for fp16 planes a power of two
 * that lifts each weight row to max |w'| in (128, 256] so that the lo plane stays in fp16's normal range.
 * In these two dtypes every convolution behind the stem (i >= 1) is stored K-TILE-MAJOR inside its block of either plane:
 * element (n, k) of [cout][k_padded] at w_off + ((k / 32) * cout + n) * 32 + k % 32 (k_padded % 32 == 0 for all of them), so
 * that a 32-deep K-tile of consecutive output channels is one contiguous run; conv 0 keeps [64][152] rows.
 * sq_resnet50_extract: give EITHER patches_u8 (uint8 NHWC [n, S, S, 3]: /255 and ImageNet
 * normalisation fused) OR patches_f32_nchw (fp32 [n, 3, S, S], already normalised: the tensor the
 * reference feeds forward_extract).  features: f32 [n, 2048].  S in {224, 256, ...}, multiple of 32.
 * ---------------------------------------------------------------------------- */
#define SQ_RESNET50_CONVS 53
typedef struct sq_conv_desc {
    int64_t w_off, b_off;
    int32_t cin, cout, k, stride, pad, k_padded;
} sq_conv_desc;
typedef struct sq_resnet50_layout {
    sq_conv_desc conv[SQ_RESNET50_CONVS];
    int64_t w_total, b_total;
} sq_resnet50_layout;
int sq_resnet50_layout_init(sq_resnet50_layout* out);
size_t sq_resnet50_workspace_bytes(int dtype, int n_patches, int patch_size);
int sq_resnet50_extract(int dtype, const void* weights, const float* bias, const uint8_t* patches_u8,
                        const float* patches_f32_nchw, int n_patches, int patch_size, float* features,
                        void* workspace, size_t workspace_bytes, sq_stream_t stream);
/* The same, with a guard for the reduced range of SQ_DTYPE_F16X3: nonfinite_flag (device word, caller-zeroed, may be NULL)
 * gets bit 0 OR-ed in when any pooled feature of this call is not finite.  An activation >= 65504 anywhere in the network
 * becomes inf planes, NaN in the next product, and the split modes' ReLU lets NaN through (csrc/x3_fmt.h), so every such
 * overflow reaches the features and the flag; the caller re-runs those patches in SQ_DTYPE_F32 (resnet.py does).
 * The reference computes src/resnet.py:155-170 in fp32, where this cannot happen below 3.4e38. */
int sq_resnet50_extract_checked(int dtype, const void* weights, const float* bias, const uint8_t* patches_u8,
                                const float* patches_f32_nchw, int n_patches, int patch_size, float* features,
                                void* workspace, size_t workspace_bytes, uint32_t* nonfinite_flag, sq_stream_t stream);
/* Rectangular and odd-sized patches: the same network on patches_u8 [n, height, width, 3] or patches_f32_nchw [n, 3, height, width].
 * Call sites: spatial_vis/visualize.py:212-216 feeds the extractor transforms.Resize((256, 265)) tiles (height 256, width 265)
 * through :62-66 into src/resnet.py:155-170, which is plain PyTorch and takes any height and width.
 * Stage sizes per axis: conv1 ceil(s/2), max-pool ceil(s/4), layers 2-4 ceil of half again, final map ceil(s/32).
 * Admitted: SQ_RESNET50_HW_MIN <= height, width <= SQ_RESNET50_HW_MAX, each independently -- exactly the sizes whose final map is
 * 7..13 per axis, where nn.AvgPool2d(7) (src/resnet.py:110,166-168) yields one (top-left) 7 x 7 window and hence [n, 2048].  Above,
 * the reference returns more than 2048 features; below, it fails.  Outside the range sq_resnet50_workspace_bytes_hw returns 0 and
 * sq_resnet50_extract_hw returns an error (sq_last_error says why) without launching anything.
 * Same weight layout, same four dtypes, same nonfinite_flag semantics as sq_resnet50_extract_checked; for height == width, a
 * multiple of 32 in [224, 416], workspace size and features are bit-identical to that entry's. */
#define SQ_RESNET50_HW_MIN 193
#define SQ_RESNET50_HW_MAX 416
size_t sq_resnet50_workspace_bytes_hw(int dtype, int n_patches, int height, int width);
int sq_resnet50_extract_hw(int dtype, const void* weights, const float* bias, const uint8_t* patches_u8,
                           const float* patches_f32_nchw, int n_patches, int height, int width, float* features,
                           void* workspace, size_t workspace_bytes, uint32_t* nonfinite_flag, sq_stream_t stream);

/* dst_bf16[i] = bf16(src[i]) -- refresh of the bf16 parameter shadow after an optimizer step.  Round to nearest, ties to even
 * (torch's .to(torch.bfloat16) bit for bit: subnormals kept, finite values beyond the bf16 range become +-inf); a NaN stays a
 * NaN, its payload and sign unspecified.
 * Alignment: both casts take any naturally aligned pointers (src 4 bytes, dst 2 bytes here; the reverse below), so any element
 * range of a flat buffer may be passed.  16-byte accesses are used when src is 16-byte and dst 8-byte aligned (below: both
 * 16-byte aligned), an element-wise kernel otherwise; the results are the same bits.
 * n == 0: nothing is launched, SQ_OK (the pointers must still be non-null).  src and dst must not overlap. */
int sq_cast_f32_to_bf16(const float* src, void* dst_bf16, size_t n, sq_stream_t stream);
/* dst[i] = fp32(src_bf16[i]) -- with the call above the pack / unpack of the bf16 gradient exchange (BASELINE config 4: "RCCL grad
 * all-reduce over xGMI, bf16"; the reference trains on one device, src/main.py:78, so there is no counterpart to cite): a gradient
 * bucket is cast to bf16, summed over the ranks in bf16 (half the ring traffic of the fp32 form), cast back into the fp32 flat
 * gradient that AdamW reads (train.py FusedTrainStep).  Exact: the bits of dst[i] are src_bf16[i] << 16, NaNs included.
 * Alignment and n == 0 as for sq_cast_f32_to_bf16. */
int sq_cast_bf16_to_f32(const void* src_bf16, float* dst, size_t n, sq_stream_t stream);

/* ------------------------------------------------------------------------------
 * Fused linear layer  C = act(A . W^T + bias + residual)   -- the nn.Linear call sites of
 * src/tformer_lin.py:14-16,37,55,57,93 and the 1x1 convolutions of src/resnet.py:60,66.
 * A [M,K] (lda) and W [N,K] (ldw) are `dtype` (f32 or bf16), bias f32 [N] or NULL,
 * residual [M,N] (ldres; res_dtype f32 or bf16) or NULL, act: 0 none, 1 exact-erf GELU, 2 ReLU,
 * C [M,N] (ldc) in out_dtype.  K, lda, ldw multiples of 16 bytes / element size.
 * workspace (optional fp32 scratch, may be NULL): lets skinny problems run split-K.
 * ---------------------------------------------------------------------------- */
int sq_linear(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual,
              int ldres, int res_dtype, int act, void* C, int out_dtype, int ldc, int M, int N, int K, void* workspace,
              size_t workspace_bytes, sq_stream_t stream);

/* Split-bf16 ("bf16x3") linear layer / convolution -- the arithmetic of SQ_DTYPE_BF16X3, exposed for the 1x1 / 3x3
 * convolutions of src/resnet.py:60-66 on caller-owned planes: every fp32 tensor is a bf16 hi plane (bf16(v)) and a
 * bf16 lo plane (bf16(v - hi)) of the same shape;  C = act(A . W^T + bias + residual) with
 * a.w = a_hi.w_hi + a_hi.w_lo + a_lo.w_hi on bf16 MFMAs, fp32 accumulation.  Output: hi / lo planes (C_hi, C_lo) or
 * fp32 (C_f32) -- give exactly one.  act: 0 none, 2 ReLU.  K, N, lda, ldw, ldc, ldres multiples of 8; planes 16-byte
 * aligned and a multiple of 16 bytes apart.  fmt: 0 = bf16 planes, 1 = fp16 planes.  colscale (optional, [N] f32): factor on
 * the accumulator column before the bias (undoes a power-of-two pre-scaling of the weight rows).  conv_geom: NULL for a plain [M,K] A, or
 * {n_img, H, W, Cin, OH, OW, KW, stride, pad} for an implicit-GEMM view of an NHWC activation (K = KH*KW*Cin, Cin % 32 == 0). */
int sq_linear_x3(int fmt, const void* A_hi, const void* A_lo, int lda, const void* W_hi, const void* W_lo, int ldw, const float* bias,
                 const float* colscale, const void* res_hi, const void* res_lo, int ldres, int act, void* C_hi, void* C_lo, float* C_f32, int ldc,
                 int M, int N, int K, const int* conv_geom, sq_stream_t stream);

/* Weight gradient of a linear layer: dW[N_out, N_in] (f32, lddw) = dY[T, N_out]^T . X[T, N_in], contracting
 * over the T token rows, straight from the token-major tensors (the `loss.backward()` of the nn.Linear call
 * sites above, src/vit.py:178).  dY (lddy) and X (ldx) are `dtype`; N_in % 8 == 0; lddy >= round_up(N_out, 8).
 * Columns [N_out, round_up(N_out, 8)) of dY must exist (the loader fetches whole 16-byte chunks) but may hold anything, NaN and
 * infinities included: a dY column only ever reaches its own row of dW and its own element of dbias, and rows >= N_out are never
 * stored (tests/test_gpu_gemm_contract.py pins this with NaN there).  Columns of dY from round_up(N_out, 8) on, columns of X from
 * N_in on and rows from n_tokens on are not read; of dW only [N_out, N_in] is written, whatever lddw.
 * dbias (optional, [N_out] f32): the bias gradient sum_t dY[t, :], computed by the same launch.
 * workspace: optional fp32 scratch enabling deterministic split-K over the tokens. */
int sq_linear_weight_grad(int dtype, const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, float* dbias,
                          int n_out, int n_in, int n_tokens, void* workspace, size_t workspace_bytes, sq_stream_t stream);
/* The same for up to FOUR same-shape layers in ONE launch (host arrays of device pointers; dbias: NULL, or one pointer per member):
 * the weight gradients of a transformer layer's linear maps (src/tformer_lin.py:18-26,54-57 under `loss.backward()`, src/vit.py:178) are
 * independent products whose 128 x 128 tile grids fill a quarter of the chip each -- together they fill it without slicing the tokens.
 * bf16 members whose extents are multiples of 128 run on the four-stage ring form of the kernel (csrc/gemm_tn.hip). */
int sq_linear_weight_grad_group(int dtype, int n_members, const void* const* dY, const void* const* X, float* const* dW,
                                float* const* dbias, int lddy, int ldx, int lddw, int n_out, int n_in, int n_tokens, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * UNI patch embedder: timm ``vit_large_patch16_224`` with ``init_values=1e-5, num_classes=0`` as
 * /root/reference/pre_processing/compute_features_hdf5.py:62-68 and spatial_vis/visualize.py:220-232 build it
 * (``feat_model(image)`` at :127-129 returns the normalised class token, [1, 1024]).  timm is not vendored in the
 * reference and absent here: the entry points follow timm's published VisionTransformer algorithm.
 *
 * sq_uni_layout: element offsets into ONE flat fp32 buffer; every timm tensor (patch_embed.proj, cls_token, pos_embed,
 * blocks.{i}.{norm1,attn.qkv,attn.proj,ls1,norm2,mlp.fc1,mlp.fc2,ls2}, norm) is a contiguous slice.
 * sq_uni_forward: params = that buffer (biases / LayerNorm / embeddings are read from it); params_exec = the same layout
 * in the compute dtype with the LayerScale gains folded into attn.proj / mlp.fc2 WEIGHTS; bias_exec = fp32 buffer of
 * the same layout whose attn.proj / mlp.fc2 BIASES carry the gains.  Give EITHER patches_u8 (uint8 NHWC [n, S, S, 3]:
 * ToTensor + Normalize of compute_features_hdf5.py:53-56 are fused in; S must equal img_size) OR patches_f32_nchw
 * (normalised, the reference's tensor).  out: f32 [n, dim].
 * Modes: SQ_DTYPE_F32 (exact), SQ_DTYPE_BF16 (fast), SQ_DTYPE_F16X3 (split fp16, the fast parity mode); SQ_DTYPE_BF16X3 is
 * refused.  SQ_DTYPE_F16X3 keeps the residual stream (patch embedding, token rows) in fp32 and carries the operands of every
 * product as fp16 hi / lo planes:
 *   params_exec: the fp16 hi plane [total] followed by the lo plane [total] of the folded weights w'[r, :] = w[r, :] s[r] of
 *                each GEMM (patch_w, qkv_w, proj_w, fc1_w, fc2_w): LayerScale is folded into proj / fc2 FIRST, then s[r] is the
 *                power of two that lifts the row's max |w'| into (128, 256] (s = 1 for a zero row);
 *   bias_exec:   fp32 [2 total]: the first half holds the folded biases as in the other modes, the second half the factors
 *                1 / s[r] at each GEMM's bias offset (patch_b, qkv_b, proj_b, fc1_b, fc2_b).
 * An fp16 overflow is not clamped: use sq_uni_forward_checked.  Launch groups: <= 1330 patches of ViT-L/16 at 224 in bf16 and
 * f16x3, <= 665 in fp32 (2 GiB buffer descriptors).
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_UNI_MAX_DEPTH 32
typedef struct sq_uni_config { int32_t dim, depth, heads, mlp_dim, img_size; } sq_uni_config;
typedef struct sq_uni_layer_offsets {
    int64_t ln1_g, ln1_b, qkv_w, qkv_b, proj_w, proj_b, ls1, ln2_g, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b, ls2;
} sq_uni_layer_offsets;
typedef struct sq_uni_layout {
    int64_t patch_w, patch_b, cls, pos, norm_g, norm_b, total;
    sq_uni_layer_offsets layer[SQ_UNI_MAX_DEPTH];
} sq_uni_layout;
int sq_uni_layout_init(const sq_uni_config* cfg, sq_uni_layout* out);
size_t sq_uni_workspace_bytes(const sq_uni_config* cfg, int dtype, int n_patches);
int sq_uni_forward(const sq_uni_config* cfg, int dtype, const float* params, const void* params_exec, const float* bias_exec,
                   const uint8_t* patches_u8, const float* patches_f32_nchw, int n_patches, float* out, void* workspace,
                   size_t workspace_bytes, sq_stream_t stream);
/* The same, with a guard for the reduced range of SQ_DTYPE_F16X3: nonfinite_flag (device word, caller-zeroed, may be NULL)
 * gets 1 ORed into it when any output feature is not finite.  Nothing saturates: an fp16 plane that overflowed anywhere
 * upstream (an activation >= 65504) reaches the class token as inf / NaN; the caller re-runs those patches in SQ_DTYPE_F32
 * (uni.py does). */
int sq_uni_forward_checked(const sq_uni_config* cfg, int dtype, const float* params, const void* params_exec, const float* bias_exec,
                           const uint8_t* patches_u8, const float* patches_f32_nchw, int n_patches, float* out, void* workspace,
                           size_t workspace_bytes, uint32_t* nonfinite_flag, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * HE2RNA comparator (/root/reference/src/he2rna.py:42-106, built by src/pretrain_gtex.py:102-105).
 * The per-tile MLP (1x1 Conv1d layers, he2rna.py:101-106) is sq_linear on the token-major tensor [B * N, C]; these
 * entry points are forward_fixed_k's masking and top-k aggregation (:93-99) and its gradient.
 *   sq_he2rna_tile_mask : mask[row] = 1 if max_c x_tokens[row, c] > 0 else 0           (:94-95; f32 [n_rows, C])
 *   sq_he2rna_topk_mean : out[b, g] = scale * sum_i  (sum_{j<k_i} sorted_desc(s[b, :, g])[j] * mask[b, j]) /
 *                         (sum_{j<k_i} mask[b, j]),   s[b, n, g] = scores[b, n, g] * mask[b, n]   (:96-98);
 *                         scale = 1 for one k (training, :85-86), 1 / len(ks) for the eval mean over ks (:88-91).
 *                         scores f32 [B, N, ld_scores >= G] token-major, N <= 128 tiles, 1 <= k_i <= N, out f32 [B, G].
 *                         0/0 (the first k tiles of a slide all masked) is NaN, as in the reference.
 *   sq_he2rna_topk_mean_bwd : grad_scores f32 [B, N, ld_grad >= G] from grad_out f32 [B, G] (columns >= G untouched).
 *   sq_he2rna_window_topk_mean : the top-k mean of sliding windows over a slide (spatial_vis/visualize.py:46-82 with
 *                         --model_type he2rna, :79-81): the MLP is per tile (1x1 convolutions, he2rna.py:101-106) and so is the mask
 *                         (:94-95), so both are computed ONCE per tile -- scores f32 [gather_rows, ld_scores >= G], mask f32
 *                         [gather_rows] -- and window w's tile n is row gather_idx[w, n] (int32 [n_windows, N]); an index outside
 *                         [0, gather_rows) is the zero padding of visualize.py:72-75 (score 0, mask 0).  out f32 [n_windows, G].
 *                         Same rank / tie rule, first-k-positions mask, fp64 sums and 0/0 = NaN as sq_he2rna_topk_mean: a
 *                         window's row is bit-identical to sq_he2rna_topk_mean on the materialised [n_windows, N, G] scores.
 * ---------------------------------------------------------------------------------------------------------- */
int sq_he2rna_tile_mask(const float* x_tokens, int n_rows, int n_channels, float* mask, sq_stream_t stream);
int sq_he2rna_topk_mean(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                        float* out, int batch, int n_tiles, int n_genes, sq_stream_t stream);
int sq_he2rna_topk_mean_bwd(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                            const float* grad_out, float* grad_scores, int ld_grad, int batch, int n_tiles, int n_genes,
                            sq_stream_t stream);
int sq_he2rna_window_topk_mean(const float* scores, int ld_scores, const float* mask, int gather_rows, const int32_t* gather_idx,
                               const int32_t* ks, int n_ks, float scale, float* out, int n_windows, int n_tiles, int n_genes,
                               sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * HE2RNA training step on the device (src/he2rna.py:108-127, the loop the k-fold experiment of :323-436 runs): fp32, one process.
 * dims = host [n_layers + 1] = {input_dim, *layers, output_dim}, n_layers <= SQ_HE2RNA_MAX_LAYERS.  Every entry is asynchronous on
 * `stream` and allocates, copies and synchronises nothing.
 *   sq_he2rna_param_layout : offsets (in floats) of layer i's weight and bias in ONE flat fp32 buffer and the buffer's size.  A weight
 *                         is [n_out, round_up(n_in, 8)] row-major; every tensor starts on a 16-byte boundary.  The padding columns and
 *                         the gaps hold zero and stay zero under the optimiser: their gradient is exactly zero, so both Adam
 *                         moments stay zero.  Gradient and moments use the same layout.  w_off / b_off / total may be NULL.
 *   sq_he2rna_loss_head : sq_he2rna_topk_mean, sq_mse_loss_grad and sq_he2rna_topk_mean_bwd of a step with each (slide, gene)
 *                         column ranked ONCE: pred f32 [B, G] (bit-identical to sq_he2rna_topk_mean), *loss_out = mean((pred -
 *                         target)^2) (device scalar, fp64 sums in a fixed order), grad_scores f32 [B, N, ld_grad >= G] = the
 *                         gradient sq_he2rna_topk_mean_bwd gives for grad_out = grad_scale * (pred - target), bit-identical; every
 *                         element of [:, :, :G] is written, zeros included, columns >= G are untouched.  grad_scores may be NULL
 *                         (forward only).  Bounds on N, k and n_ks as sq_he2rna_topk_mean.  The ranking and the gradient are one
 *                         launch; a one-block launch behind it adds the blocks' partial sums of the loss.
 *   sq_he2rna_dropout   : in place on act f32 [rows, ld], columns < width: an element is kept when u >= p and scaled by 1 / (1 - p).
 *                         u in [0, 1) is word (column % 4) of Philox4x32-10 with key = seed on the counter (column / 4, row, layer,
 *                         step): a pure function of (seed, step, layer, row, column), whatever the grid.  p = 0 launches nothing;
 *                         p >= 1 is refused.  0 <= step < 2^32.
 *   sq_he2rna_dropout_gate : grad[r, c] = act[r, c] > 0 ? grad[r, c] / (1 - p) : 0 for c < width, in place: ReLU and dropout backward
 *                         from the saved post-dropout activation, no stored mask.  16-byte accesses when both tables allow them,
 *                         a scalar tail for widths that are no multiple of 4.
 *   sq_he2rna_train_forward : x f32 [B * N, C] token-major (the loader's layout); the tile mask is taken over all C channels, the
 *                         model reads the last dims[0].  Layer stack from the flat buffer (sq_linear, bias and ReLU in the
 *                         epilogue), dropout behind every hidden layer (layer = its index), then the loss head with
 *                         grad_scale.  Saves the padded input, every layer's output and the gradient of the scores in the
 *                         workspace: sq_he2rna_train_workspace_bytes gives its size and, in act_offsets (NULL or [n_layers + 1]),
 *                         where the input (0) and layer i's output (i + 1) lie, in floats from its start, as [B * N,
 *                         round_up(width, 8)] tables.
 *   sq_he2rna_train_backward : the flat gradient of the loss sq_he2rna_train_forward left in the SAME workspace (same dims, B, N,
 *                         p_drop, params): sq_linear_weight_grad with the bias sums, dX as NT products on transposed weight copies
 *                         made here, sq_he2rna_dropout_gate between them.  The input gets no gradient.  Every element of every
 *                         tensor of `grads` is written; the gaps between tensors are not.
 * The optimiser of the step is sq_adamw_step with weight_decay = 0: torch.optim.Adam(lr, weight_decay=0.) term for term.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_HE2RNA_MAX_LAYERS 8
int sq_he2rna_param_layout(const int32_t* dims, int n_layers, int64_t* w_off, int64_t* b_off, int64_t* total);
size_t sq_he2rna_loss_head_workspace_bytes(int batch, int n_genes);
int sq_he2rna_loss_head(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                        const float* target, float grad_scale, float* pred, float* loss_out, float* grad_scores, int ld_grad,
                        int batch, int n_tiles, int n_genes, void* workspace, size_t workspace_bytes, sq_stream_t stream);
int sq_he2rna_dropout(float* act, int ld, int rows, int width, float p, long long seed, long long step, int layer,
                      sq_stream_t stream);
int sq_he2rna_dropout_gate(float* grad, int ld_grad, const float* act, int ld_act, int rows, int width, float p,
                           sq_stream_t stream);
size_t sq_he2rna_train_workspace_bytes(const int32_t* dims, int n_layers, int batch, int n_tiles, int64_t* act_offsets);
int sq_he2rna_train_forward(const float* x, int batch, int n_tiles, int n_channels, const int32_t* dims, int n_layers,
                            const float* params, const int32_t* ks, int n_ks, float scale, float p_drop, long long seed,
                            long long step, const float* target, float grad_scale, float* pred, float* loss_out, void* workspace,
                            size_t workspace_bytes, sq_stream_t stream);
int sq_he2rna_train_backward(int batch, int n_tiles, const int32_t* dims, int n_layers, const float* params, float p_drop,
                             float* grads, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Pillow-exact resize of uint8 patches (the resize in front of the extractors: `transforms.Resize(224)` on a PIL image,
 * /root/reference/pre_processing/compute_features_hdf5.py:53-56,125-126 and spatial_vis/visualize.py:226-230, which is
 * Image.resize(..., BILINEAR); `patch.resize(patch_size)`, pre_processing/patch_gen_hdf5.py:117, Pillow's default BICUBIC).
 * Pillow's resampler (src/libImaging/Resample.c) is deterministic integer arithmetic on per-axis coefficient tables, and
 * these entry points restate it bit for bit: two separable passes, horizontal then vertical, through a uint8
 * intermediate image (the rounding between the passes is part of the result); a pass whose input and output extents are
 * equal is the identity.  Per axis in -> out: scale = in / out, filterscale = max(scale, 1), support = S * filterscale
 * (S = 1 bilinear, 2 bicubic), ksize = 2 ceil(support) + 1; output index xx takes the input samples [xmin, xmin + n) around
 * center = (xx + 0.5) scale with weights f((x + xmin - center + 0.5) / filterscale), normalised to sum 1 in double and
 * rounded to 22 fractional bits; out = clamp((2^21 + sum k[i] src[xmin + i]) >> 22, 0, 255) in int32.
 *
 * The tables are data-independent double arithmetic, so they are made on the HOST, once per
 * (h_in, w_in, h_out, w_out, filter), and uploaded by the caller (like the *_layout_init entries, no device work):
 *   sq_resize_plan_bytes : size of the plan in bytes; 0 (and an sq_last_error message) for sizes outside 1..16384 or an
 *                          unknown filter.
 *   sq_resize_plan_init  : fills `plan` (host memory, plan_bytes >= sq_resize_plan_bytes) with int32 words:
 *                            [0..7]  h_in, w_in, h_out, w_out, filter, ksize_h, ksize_v, 0
 *                            horizontal pass (w_in -> w_out): bounds [w_out][2] = {xmin, n}, then coefficients
 *                            [w_out][ksize_h] (22 fractional bits, zero beyond n)
 *                            vertical pass (h_in -> h_out): bounds [h_out][2], then coefficients [h_out][ksize_v]
 *                          An identity pass has ksize 1: bounds {xx, 1}, coefficient 2^22.
 *   sq_resize_u8         : src_u8 uint8 NHWC [n, h_in, w_in, 3] -> dst_u8 uint8 NHWC [n, h_out, w_out, 3] with the uploaded
 *                          plan of exactly these sizes and filter (device memory, 4-byte aligned).  One launch; the
 *                          intermediate image lives in LDS.  Sizes whose narrowest band of rows does not fit the 160 KiB
 *                          of LDS (very wide images under a large reduction) are refused with the byte count.
 *   sq_resize_u8_gather  : the same kernels, plan and bytes with a gather in front and 3 or 4 bytes per source pixel:
 *                          src_u8 uint8 [n_src, h_in, w_in, pixel_bytes] (pixel_bytes 3, or 4 = RGBA with the fourth byte
 *                          ignored and the base 4-byte aligned) -> dst_u8 uint8 [m, h_out, w_out, 3], dst[j] = the resize of
 *                          src[index[j]].  index: int32 [m] in device memory, or null for the identity with m = n_src.  An
 *                          index outside [0, n_src) gives an all-zero image (it is compared before it addresses anything).
 *                          m = 0 launches nothing.  sq_resize_u8 is its call with pixel_bytes 3 and a null index.
 *   sq_pack_rgb_gather   : the same gather without a resize: src_u8 [n_src, h, w, pixel_bytes] -> dst_u8 [m, h, w, 3] dense
 *                          RGB, dst[j] = src[index[j]][..., :3]; extents in 1..SQ_RESIZE_MAX_DIM; index, out-of-range
 *                          entries and m = 0 as above.  Dword loads and stores where a tile starts dword-aligned.
 *                          Both are asynchronous on `stream`; arguments are checked before the launch.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_RESIZE_BILINEAR 0 /* PIL.Image.BILINEAR */
#define SQ_RESIZE_BICUBIC 1  /* PIL.Image.BICUBIC, a = -0.5 */
#define SQ_RESIZE_MAX_DIM 16384
size_t sq_resize_plan_bytes(int h_in, int w_in, int h_out, int w_out, int filter);
int sq_resize_plan_init(int h_in, int w_in, int h_out, int w_out, int filter, int32_t* plan, size_t plan_bytes);
int sq_resize_u8(const uint8_t* src_u8, int n, int h_in, int w_in, uint8_t* dst_u8, int h_out, int w_out, int filter,
                 const int32_t* plan_dev, sq_stream_t stream);
int sq_resize_u8_gather(const uint8_t* src_u8, int n_src, int pixel_bytes, const int32_t* index, int m, int h_in, int w_in,
                        uint8_t* dst_u8, int h_out, int w_out, int filter, const int32_t* plan_dev, sq_stream_t stream);
int sq_pack_rgb_gather(const uint8_t* src_u8, int n_src, int pixel_bytes, const int32_t* index, int m, int h, int w,
                       uint8_t* dst_u8, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Patch filter: the per-tile tissue and contrast test of patch generation
 * (/root/reference/pre_processing/patch_gen_hdf5.py:25-38,110-115: get_mask_image, binary_dilation(iterations=3), the
 * tissue count against background_threshold, skimage.exposure.is_low_contrast) for a batch of uint8 tiles, with the
 * arithmetic of sequoia-pub_amd/patchgen.py.  Per tile, everything in IEEE double, one rounding per operation, no fused
 * multiply-add:
 *   Otsu of R, G, B     256 counts; bins lo..hi of the channel with the integers as centres; per split i: weight1 = counts
 *                       up to i, weight2 = counts beyond, mean1/2 = sum(counts centre) / weight, variance12 =
 *                       (weight1 weight2) ((mean1 - mean2) (mean1 - mean2)); the first maximum wins; a constant channel
 *                       returns its value.
 *   saturation s        c = fl(u8 (1 / 255.0)) per channel, v = max, delta = max - min, s = delta / v, 0 where delta == 0.
 *   Otsu of s           256 bins over [min s, max s]: edge[i] = fl(fl(i step) + min), step = (max - min) / 256, edge[256] =
 *                       max; s is in bin i when edge[i] <= s < edge[i + 1], the last bin closed; centres
 *                       (edge[i] + edge[i + 1]) / 2; the cumulative sums of counts centre run sequentially, forward and
 *                       backward (np.cumsum); constant s returns the value.
 *   mask                s > thr_S and not (R > thr_R and G > thr_G and B > thr_B) and R, G, B > rgb_min.
 *   dilation            three iterations of the cross, zero outside the tile (scipy's default binary_dilation).
 *   tissue              dilated_count > fl(background_threshold (double)(h w)).
 *   contrast_ratio      (p99 - p1) / 2 of the luminance 0.2125 R + 0.7154 G + 0.0721 B of the pixels / 255, numpy's linear
 *                       percentiles.  numpy forms the luminance through BLAS, whose last bit is not defined by a fixed
 *                       order, so this value alone is defined to 1e-12, not to the bit: the order statistics are selected
 *                       by the integer key 2125 R + 7154 G + 721 B and the luminance is key / 2550000.
 *   keep                tissue and not (contrast_ratio < contrast_fraction).
 *
 *   sq_patch_filter_workspace_bytes : bytes of workspace for n tiles of h x w; 0 (and an sq_last_error message) for n < 1
 *                          or an extent outside 8..512 (512 = the 40x read of a 256-pixel patch; the cap keeps a tile's
 *                          h w mask bits in LDS).  The workspace receives the result rows when `stats` is null.
 *   sq_patch_filter      : patches_u8 uint8 NHWC [n, h, w, 3] (any alignment) -> keep uint8 [n] (0 / 1); stats double [n, 8]
 *                          or null: thr_R, thr_G, thr_B, thr_S, mask_count, dilated_count, contrast_ratio, 0 (the counts are
 *                          exact); mask_raw / mask_dilated uint8 [n, h, w] (0 / 1), each may be null.  One launch, one
 *                          workgroup per tile, asynchronous on `stream`; arguments are checked before the launch.
 *   sq_patch_filter_px   : the same with pixel_bytes bytes per pixel: 3 is sq_patch_filter; 4 takes [n, h, w, 4] (RGBA as a
 *                          slide reader returns it), the base 4-byte aligned, the fourth byte of every pixel ignored.  Only
 *                          the load differs (whole dwords, nothing staged): every output equals the 3-byte call on the same
 *                          RGB values bit for bit.  The workspace does not depend on pixel_bytes.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_PATCH_FILTER_MIN_DIM 8
#define SQ_PATCH_FILTER_MAX_DIM 512
size_t sq_patch_filter_workspace_bytes(int n, int h, int w);
int sq_patch_filter(const uint8_t* patches_u8, int n, int h, int w, int rgb_min, double background_threshold,
                    double contrast_fraction, uint8_t* keep, double* stats, uint8_t* mask_raw, uint8_t* mask_dilated,
                    void* workspace, size_t workspace_bytes, sq_stream_t stream);
int sq_patch_filter_px(const uint8_t* patches_u8, int n, int h, int w, int pixel_bytes, int rgb_min, double background_threshold,
                       double contrast_fraction, uint8_t* keep, double* stats, uint8_t* mask_raw, uint8_t* mask_dilated,
                       void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Slide mask: the whole-slide tissue mask of patch generation and its closing
 * (pre_processing/patch_gen_hdf5.py:25-50,69-72: get_mask_image on the lowest pyramid level, then
 * binary_dilation(iterations=3) and binary_erosion(iterations=3)) for ONE uint8 image of any size.  Thresholds, saturation
 * and mask are those of "Patch filter" above, operation for operation (one set of device functions serves both), so the
 * four thresholds and every mask bit equal the host's.  The closing is `iterations` steps of the cross and then as many
 * of its erosion, both with zeros outside the image (scipy's defaults: border_value = 0 -- an all-ones image comes back
 * with a frame of `iterations` zeros).  The cross is symmetric, so mask and closing commute with transposing the image;
 * `transpose` writes both byte outputs as [w, h], which is the [x, y] layout of the reference's mask.npy.
 * Several passes over a grid of workgroups; whatever is combined across workgroups is an integer count or a min / max,
 * so two calls give the same bytes.
 *
 *   sq_slide_mask_workspace_bytes : bytes of workspace for an h x w image (histograms, thresholds, a bit image of
 *                          ceil(w / 32) words per row); 0 (and an sq_last_error message) for an extent outside
 *                          1..SQ_SLIDE_MASK_MAX_DIM or h w > 2^30: pixel counts and the histograms' totals are kept in 32
 *                          bits (counts x centre sums then stay below 2^53, as the Otsu walks need).
 *   sq_slide_mask        : img_u8 uint8 [h, w, 3] (any alignment) -> mask_closed uint8 [h, w] (0 / 1), or [w, h] when
 *                          `transpose` is not 0; mask_raw the same for the mask before the closing, or null; stats double
 *                          [8] or null: thr_R, thr_G, thr_B, thr_S, raw count, closed count, min s, max s (all exact).
 *                          iterations in 0..SQ_SLIDE_MASK_MAX_ITERATIONS (the reference: 3); with 0 the closed mask is the
 *                          raw one.  Arguments are checked before anything is launched; the call clears the part of the
 *                          workspace it needs cleared on `stream`, is asynchronous on it and never synchronises.
 *                          The closing works on tiles of SQ_SLIDE_MASK_TILE_ROWS x SQ_SLIDE_MASK_TILE_COLS mask bits.
 *   sq_slide_mask_px     : the same with pixel_bytes bytes per pixel: 3 is sq_slide_mask; 4 takes [h, w, 4], the base 4-byte
 *                          aligned, the fourth byte ignored; same bounds, workspace and bytes out.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_SLIDE_MASK_MAX_DIM 32768
#define SQ_SLIDE_MASK_MAX_ITERATIONS 8
#define SQ_SLIDE_MASK_TILE_ROWS 64
#define SQ_SLIDE_MASK_TILE_COLS 256
size_t sq_slide_mask_workspace_bytes(int h, int w);
int sq_slide_mask(const uint8_t* img_u8, int h, int w, int rgb_min, int iterations, int transpose,
                  uint8_t* mask_raw, uint8_t* mask_closed, double* stats,
                  void* workspace, size_t workspace_bytes, sq_stream_t stream);
int sq_slide_mask_px(const uint8_t* img_u8, int h, int w, int pixel_bytes, int rgb_min, int iterations, int transpose,
                     uint8_t* mask_raw, uint8_t* mask_closed, double* stats,
                     void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tile grid: which grid tiles of a slide the spatial maps read
 * (spatial_vis/visualize.py:174-205, restated on the host by cli/visualize.py valid_tiles: a double loop over the grid,
 * scipy's binary_dilation(iterations=3) of a window of the tissue mask per tile, its count against half the window).
 * The mask is the array of mask.npy: uint8 [mask_w, mask_h], C-contiguous, indexed [x, y], any non-zero byte is tissue.
 * For grid tile (i, j), 0 <= i < n_col, 0 <= j < n_row, with the read size p (patch_size_resized) and the downsample
 * factor ds of the mask:
 *   origin              col = i p, row = j p in level-0 pixels; the host takes n_col = len(range(0, slide_w - p, p)) and
 *                       n_row likewise, the caller passes both.
 *   window              c = col / ds, r = row / ds in integer division -- equal to the host's int(col / downsample_factor),
 *                       a double division, for every extent below 2^31 (the quotient's rounding error stays below 1 / ds);
 *                       x in [c, min(c + pm, mask_w)), y in [r, min(r + pm, mask_h)): clipped as numpy slicing clips it, on
 *                       either axis, and EMPTY for pm = 0 or an origin beyond the mask (the two axes of a pyramid level
 *                       may have been truncated differently).
 *   dilation            `iterations` steps of the cross INSIDE the window, zeros outside it (scipy's border_value = 0 on
 *                       the slice): a mask pixel next to the window does not enter.  Inside a rectangle that is "L1
 *                       distance <= iterations to a set pixel of the window".  The cross is symmetric, so the window is
 *                       walked in the mask's [x, y] layout, untransposed.
 *   size, count         the clipped window's element count; the set pixels after the dilation.
 *   valid               (double)count >= fl(threshold (double)size): with threshold 0.5 a tie 2 count == size is valid, and
 *                       an empty window is valid (0 >= 0, as scipy and the host loop have it).
 *
 *   sq_tile_grid_valid   : mask_u8 (any alignment) -> valid uint8 [n_col, n_row] (0 / 1; n_col is the outer axis, the host's
 *                          visiting order); counts and sizes int32 [n_col, n_row], each may be null.  mask_w, mask_h in
 *                          1..SQ_TILE_GRID_MAX_DIM and mask_w mask_h <= 2^30 (the slide mask's bounds; addresses are formed
 *                          in 64 bits); n_col, n_row >= 1, n_col n_row <= 2^30 and every tile origin below 2^31; p, ds >= 1;
 *                          pm in 0..SQ_TILE_GRID_MAX_WINDOW (512 = a 40x read with a full-resolution mask; the cap keeps a
 *                          window's bits in LDS, as the patch filter's does); iterations in
 *                          0..SQ_TILE_GRID_MAX_ITERATIONS (the reference: 3, threshold 0.5).  One launch: windows up to
 *                          SQ_TILE_GRID_PACKED_MAX_WINDOW take the packed route (a window row is one 32- or 64-bit word of
 *                          a lane, 8 to 1 windows per wave), wider ones one workgroup each with the bits in LDS.  All
 *                          arguments are checked before the launch; asynchronous on `stream`, never synchronises; every
 *                          window is independent and every sum an integer, so two calls give the same bytes.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_TILE_GRID_MAX_DIM 32768
#define SQ_TILE_GRID_MAX_WINDOW 512
#define SQ_TILE_GRID_PACKED_MAX_WINDOW 64
#define SQ_TILE_GRID_MAX_ITERATIONS 8
int sq_tile_grid_valid(const uint8_t* mask_u8, int mask_w, int mask_h, int n_col, int n_row, int p, int ds, int pm,
                       int iterations, double threshold, uint8_t* valid, int32_t* counts, int32_t* sizes,
                       sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Map statistics: what spatial_vis/gbm_celltype_analysis.py and the percentile step of spatial_vis/get_emd.py compute
 * from a slide's prediction table (f32 [n_tiles, G], as spatial.sliding_window_all_genes leaves it on the device).
 * Tables are row-major with a leading dimension `ld` (elements); `cols` is a device list of int32 column indices in
 * [0, ld), NULL = columns 0..C-1 (C <= ld): gene columns are read in place.  n <= SQ_MAP_MAX_ROWS tiles.  Every argument
 * is checked before the first launch; the calls are asynchronous on `stream` and never synchronise; no floating-point
 * atomics, every sum in a fixed order: two calls give the same bytes.
 * Invariant of every *_workspace_bytes function here and under "Ground-truth alignment": it returns 0 exactly when one
 * of its own arguments is outside the range its entry admits, the entry then refuses the same arguments with SQ_ERR_ARG,
 * and every refusal precedes the first launch.  A caller need not test the size: it makes the call with non-null
 * pointers and a workspace of at least that size (any, if 0), and the entry's own message says what is wrong.
 *
 *   sq_map_percentile   : score2percentile of gbm_celltype_analysis.py:12-16,107 and get_emd.py:21-25,172,175 for every
 *                         element of every column: scipy.stats.percentileofscore(column, x) with the default kind='rank',
 *                         (left + right + (left < right)) * (50.0 / n) with left = #(column < x), right = #(column <= x) as
 *                         integers and ONE f64 product; `scale` is the caller's 50.0 / n.  Bit-equal to scipy.  values is
 *                         f32 (values_f64 = 0) or f64 (1); out f64 [n, C].  Comparisons are IEEE (-0.0 == 0.0, +-inf
 *                         ordered).  A column holding a NaN comes back all NaN (nan_policy='propagate').  argmax, when
 *                         not NULL, is int32 [n]: the first column holding the row's largest percentile, NaN skipped, -1
 *                         for a row of NaN (df[[... '_perc']].idxmax(axis=1) of :109, ties to the earlier column).
 *                         1 <= n <= SQ_MAP_MAX_ROWS, C >= 1.  A column is cut into chunks of sq_map_rank_chunk_rows()
 *                         rows; one workgroup sorts a chunk's keys in LDS (csrc/colsort.hip, shared with
 *                         sq_gt_count_unique), every element is then searched in every sorted chunk of its column with the
 *                         lower- and upper-bound search of csrc/colsort.h (counts add over chunks).
 *   sq_map_category_means : df[genes of a category].mean(axis=1) of :105.  pred f32 [n, ld]; members int32 [offsets[n_cat]]
 *                         gene (column) indices, category c owns members[offsets[c] .. offsets[c + 1]) (both on the device,
 *                         indices in [0, ld) -- the caller validates them); out f64 [n, n_cat] = the f64 sum of the
 *                         members in list order divided by their count, NaN for an empty category (as pandas).
 *                         1 <= n <= SQ_MAP_MAX_ROWS, n_cat >= 1, n_members >= 0.
 *   sq_map_gene_corr    : df[all_genes].corr() of :75 (Pearson) for K columns of pred f32 [n, ld]: out f64 [K, K].  Column
 *                         means in f64, C = Z^T Z of the centred columns over the n rows on v_mfma_f64_16x16x4_f64 (blocks on
 *                         and above the diagonal only, the rows cut into slices whose partials are added in slice order),
 *                         out[i][j] = C_ij / (sqrt(C_ii) sqrt(C_jj)) clipped to [-1, 1] and stored at [i][j] and [j][i]
 *                         (bit-symmetric); the diagonal is exactly 1.0.  A constant column (every value equal to the
 *                         first) gives NaN in its row and column, the diagonal included (as pandas).  A NaN VALUE makes
 *                         its column's row and column NaN (pandas would drop the pair's rows: not done here, the tables
 *                         of :72 have had their NaN rows dropped).  2 <= n <= SQ_MAP_MAX_ROWS, 1 <= K <= SQ_MAP_MAX_CORR_COLS.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_MAP_MAX_ROWS 262144
#define SQ_MAP_MAX_CORR_COLS 32768
int sq_map_rank_chunk_rows(void);
size_t sq_map_percentile_workspace_bytes(int n, int C, int values_f64);
int sq_map_percentile(const void* values, int values_f64, int n, int ld, const int32_t* cols, int C, double scale,
                      double* out, int32_t* argmax, void* workspace, size_t workspace_bytes, sq_stream_t stream);
int sq_map_category_means(const float* pred, int n, int ld, const int32_t* members, int n_members, const int32_t* offsets,
                          int n_cat, double* out, sq_stream_t stream);
size_t sq_map_gene_corr_workspace_bytes(int n, int K);
int sq_map_gene_corr(const float* pred, int n, int ld, const int32_t* cols, int K, double* out, void* workspace,
                     size_t workspace_bytes, sq_stream_t stream);

/* Map statistics, the cluster map: sns.clustermap(corrdf) of gbm_celltype_analysis.py:81,145 reorders the correlation
 * matrix by scipy.cluster.hierarchy.linkage(corrdf.values, method='average', metric='euclidean') and the leaf order of its
 * dendrogram.  The two entries compute that for B problems of one shape per call, bit for bit as scipy does, under the
 * conventions above (every argument checked before the first launch, *_workspace_bytes 0 exactly for the refused
 * arguments, asynchronous, no floating-point atomics, two calls give the same bytes).  2 <= K <= SQ_MAP_MAX_LINK_ROWS (what
 * one workgroup's LDS holds of the chain, the cluster sizes, the union-find parents and the sort keys),
 * 1 <= B <= SQ_MAP_MAX_LINK_BATCH, 1 <= M <= SQ_MAP_MAX_ROWS.
 *
 *   sq_map_row_distances   : pdist(A, 'euclidean') of B matrices a f64 [B, K, ld] of K observations x M features (M <= ld):
 *                         dist f64 [B, K, K], symmetric (each pair computed once and stored on both sides), the diagonal
 *                         exactly 0.  Per pair scipy's loop: s = 0; for t = 0 .. M-1: d = a[i][t] - a[j][t]; s = s + d d, the
 *                         product and the sum rounded separately (no FMA), then sqrt(s).  status int32 [B]: 0, or 1 + the
 *                         smallest row that has a distance to another row that is not finite (scipy's linkage raises
 *                         ValueError there).
 *   sq_map_linkage_average : scipy's nn_chain for method='average' on dist f64 [B, K, K] (symmetric, as above; OVERWRITTEN),
 *                         one workgroup per problem.  A nearest-neighbour chain: from the chain's top x the nearest live
 *                         cluster (the element below x in the chain on ties with it, otherwise the smallest index); a
 *                         reciprocal pair a < b is merged at that distance: a dies, b takes na + nb members and
 *                         D[i][b] = D[b][i] = (na D[i][a] + nb D[i][b]) / (na + nb) for every live i (two products, a sum and
 *                         a quotient, each rounded); an empty chain restarts from the live cluster of smallest index.  The
 *                         K - 1 merges, sorted stably by distance and relabelled by a union-find over 2K - 1 labels, are
 *                         Z f64 [B, K-1, 4] = (smaller root, larger root, distance, members), row r creating label K + r;
 *                         leaves int32 [B, K] is the depth-first walk from label 2K - 2, column 0 first: leaves_list(Z),
 *                         dendrogram(Z, no_plot=True)['leaves'].  dist_status (NULL: none) is sq_map_row_distances' status:
 *                         a problem whose word is not 0 is left alone (SQ_LINK_NONFINITE; Z, leaves and dist untouched).
 *                         With or without it every search checks the row it reads on the device: a distance to a live
 *                         cluster that is NaN, infinite or negative ends the problem with SQ_LINK_BAD_DISTANCE before any
 *                         index is derived from it (Z and leaves untouched, dist partly merged), so a matrix nobody has
 *                         checked cannot send the kernel outside its buffers.
 *                         Bounded work: a chain makes at most 3 (K - 1) searches; the kernel counts them and ends the problem
 *                         with SQ_LINK_SEARCH_BOUND past that.  status int32 [B], always written.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_MAP_MAX_LINK_ROWS 4096
#define SQ_MAP_MAX_LINK_BATCH 65535
#define SQ_LINK_OK 0
#define SQ_LINK_NONFINITE 1            /* the problem's dist_status word was not 0: nothing was computed */
#define SQ_LINK_SEARCH_BOUND 2         /* more than 3 (K - 1) nearest-neighbour searches */
#define SQ_LINK_BAD_DISTANCE 3         /* a search met a distance that is NaN, infinite or negative */
size_t sq_map_row_distances_workspace_bytes(int B, int K, int M);
int sq_map_row_distances(const double* a, int B, int K, int M, int ld, double* dist, int32_t* status, void* workspace,
                         size_t workspace_bytes, sq_stream_t stream);
size_t sq_map_linkage_average_workspace_bytes(int B, int K);
int sq_map_linkage_average(double* dist, int B, int K, const int32_t* dist_status, double* Z, int32_t* leaves, int32_t* status,
                           void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ground-truth alignment: what spatial_vis/get_emd.py computes between a predicted slide and its spatial-transcriptomics
 * spots before the EMD -- get_average (:27-38), median_filter (:41-51) and the np.unique counts of :204-205; the
 * percentile step (:21-25,172,175) is sq_map_percentile above.  Tables are row-major with a leading dimension `ld` and an
 * optional device list `cols` of int32 column indices, as in the map statistics.  Every argument is checked before the
 * first launch; the calls are asynchronous on `stream` and never synchronise; no floating-point atomics, every sum in a
 * fixed order: two calls give the same bytes.  Everything is integer work or a separately rounded f64 operation in a
 * defined order (no fused multiply-add, a correctly rounded square root), so the results equal the reference's own
 * calls bit for bit; the sign and payload of a NaN are not part of that.
 *
 *   sq_gt_nearest_spots : get_average's `sorted(range(n_spots), key=distances)[:num_tiles]` (:29-32) for every tile at once.
 *                         xc, yc f64 [n_tiles] tile coordinates, sx, sy f64 [n_spots] spot coordinates;
 *                         d = sqrt((sx - xc)(sx - xc) + (sy - yc)(sy - yc)).  idx int32 [n_tiles, k_eff], k_eff =
 *                         min(k, n_spots): the first k_eff spots of a STABLE sort by d -- equal d goes to the lower spot
 *                         index, and equality is judged on d, not on d^2 -- in that order; dist, when not NULL, f64 of the
 *                         same shape.  1 <= n_tiles <= SQ_MAP_MAX_ROWS, 1 <= n_spots <= SQ_GT_MAX_SPOTS,
 *                         1 <= k <= SQ_GT_MAX_K.  NaN coordinates are the caller's to refuse (Python's sorted has no
 *                         defined order for them).  One thread per tile, the spots staged through LDS in chunks of
 *                         sq_gt_spot_chunk(), the k best in registers.
 *   sq_gt_spot_means    : np.mean of the kept spots' expression (:34-38).  idx int32 [n_tiles, k_eff] as above; expr f32
 *                         (expr_f64 = 0; widened to f64 first) or f64 (1) [n_spots, ld]; out f64 [n_tiles, C] =
 *                         (((0.0 + e0) + e1) + ...) / k_eff in kept order for k_eff <= 7 and numpy's pairwise block
 *                         (0.0 + (((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)))) / 8 for k_eff = 8.  A NaN or an
 *                         infinity propagates.  A spot index outside [0, n_spots) is not followed: that mean is NaN.
 *   sq_gt_median_filter : median_filter(df, col, x, y, r) (:41-51) for every row of every column.  values f64 [n, ld];
 *                         xtf, ytf int32 [n] grid coordinates in [0, grid_w) x [0, grid_h), grid_w grid_h <=
 *                         SQ_GT_MAX_GRID_CELLS; r in 1..SQ_GT_MAX_RADIUS.  The window of a row is the rows with
 *                         |xtf - x| <= r and |ytf - y| <= r, c of them; if 2 c > (2 r + 1)^2 the result is np.median of
 *                         the window -- NaN if a member is NaN, else 0.0 + the middle of the sorted members (odd c) or
 *                         ((0.0 + a) + b) / 2.0 of the two middle ones (even c), infinities and overflow as that
 *                         expression has them -- otherwise the row's own value.  nan_absent = 1: a NaN in column c means
 *                         the row is absent from column c (the per-gene dropna of :166): it is counted in no window of
 *                         that column and its own result is NaN.  out f64 [n, C]; counts, when not NULL, int32 [n, C]:
 *                         the windows' c.  Two rows in one grid cell are not supported: `flag`, one caller-zeroed
 *                         device byte, is set to 1 when a row does not find its own number in its cell or a coordinate
 *                         lies outside the grid (such a row reads nothing and its result is NaN); the results are then
 *                         not to be used.  A first kernel scatters the row numbers into the workspace's int32 grid, a
 *                         second sorts each window in a per-thread column of LDS.
 *   sq_gt_count_unique  : len(np.unique(column)) (:204-205) of C columns of values f64 [n, ld]: out int32 [C].  -0.0 and
 *                         0.0 are one value, all NaNs together are one.  1 <= n <= SQ_MAP_MAX_ROWS,
 *                         1 <= C <= SQ_GT_MAX_UNIQUE_COLS.  Chunks of sq_gt_unique_chunk_rows() rows (the percentile's
 *                         chunk: sq_map_rank_chunk_rows()) are sorted in LDS by the percentile's kernel (csrc/colsort.hip); a
 *                         value counts in the first chunk that holds it, found with the lower-bound search of csrc/colsort.h.
 *   The two *_workspace_bytes functions return 0 exactly for the refused shapes (the invariant stated above).
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_GT_MAX_SPOTS 1048576
#define SQ_GT_MAX_K 8
#define SQ_GT_MAX_RADIUS 3
#define SQ_GT_MAX_GRID_CELLS 16777216
#define SQ_GT_MAX_UNIQUE_COLS 65536
int sq_gt_spot_chunk(void);
int sq_gt_unique_chunk_rows(void);
int sq_gt_nearest_spots(const double* xc, const double* yc, int n_tiles, const double* sx, const double* sy, int n_spots, int k,
                        int32_t* idx, double* dist, sq_stream_t stream);
int sq_gt_spot_means(const int32_t* idx, int n_tiles, int k_eff, const void* expr, int expr_f64, int n_spots, int ld,
                     const int32_t* cols, int C, double* out, sq_stream_t stream);
size_t sq_gt_median_filter_workspace_bytes(int n, int grid_w, int grid_h);
int sq_gt_median_filter(const double* values, int n, int ld, const int32_t* cols, int C, const int32_t* xtf, const int32_t* ytf,
                        int grid_w, int grid_h, int r, int nan_absent, double* out, int32_t* counts, uint8_t* flag,
                        void* workspace, size_t workspace_bytes, sq_stream_t stream);
size_t sq_gt_count_unique_workspace_bytes(int n, int C);
int sq_gt_count_unique(const double* values, int n, int ld, const int32_t* cols, int C, int32_t* out, void* workspace,
                       size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Earth mover's distance: the number spatial_vis/get_emd.py exists for (get_emd.py:54-90,180-189) -- the grid fill and
 * shift of :180-188, calculate_emd's conventions and normalisation (:71-82) and, in place of cv2.EMD (:86), the optimum of
 * the balanced transportation problem between the two weighted cell sets, in f64, with an optimality certificate: a
 * feasible flow and feasible duals of equal objective.  cv2.EMD casts its signatures to float32 and stops at its own
 * epsilon: it approximates this number and does not define it.  P independent problems per call, ONE WORKGROUP PER
 * PROBLEM, no workgroup ever waits on another; every sum in a fixed order, no floating-point atomics: two calls give the
 * same bytes.  Every argument is checked before the first launch; the calls are asynchronous on `stream` and never
 * synchronise.  sq_emd_workspace_bytes keeps the invariant stated under "Map statistics".
 * Every pointer is a device pointer, with ONE exception: sq_emd_status_check reads the statuses from HOST memory (the
 * caller has downloaded them, which is the synchronisation the entries themselves never make) and only formats
 * sq_last_error.
 *
 *   sq_emd_fill  : :180-188 for P problems over one slide's table rows.  Problem p compares column cols_a[p] of a f64
 *                  [n, lda] with column cols_b[p] of b f64 [n, ldb] (NULL: column p); xtf, ytf int32 [n] grid coordinates
 *                  in [0, grid_h) x [0, grid_w) (arr[x, y]: x indexes the grid's rows).  nan_absent = 1: a row that is NaN
 *                  in either column is absent from that problem (the per-gene dropna of :166).  Over the present rows:
 *                  H = max x + 1, W = max y + 1 -> dims[p] = (H, W); both grids start from zeros, arr[x, y] = value, then
 *                  arr + abs(min(arr)) with the min over the WHOLE H x W grid, empty cells included -- with a negative
 *                  minimum every empty cell becomes positive; literal, not guarded.  grids f64 [P, 2, cells] (cells >=
 *                  grid_h grid_w, row-major H_p x W_p at the front of each plane).  No present row: dims (0, 0).  Two
 *                  present rows in one cell, or a coordinate outside the grid, set the caller-zeroed byte flag[0]; the
 *                  results are then not to be used.  workspace: P cells int32 (the owners' row numbers).
 *   sq_emd_solve : calculate_emd (:67-90) for P pairs of dense non-negative f64 grids [P, 2, cells] with dims int32 [P, 2]
 *                  = (H_p, W_p), H_p, W_p <= SQ_EMD_MAX_DIM (a device-side check; status below).  Both grids all zero ->
 *                  0.0; exactly one -> NaN (:71-79; an empty grid is all zero).  Otherwise each grid is divided by its f64
 *                  sum and the cells with weight > 0 are kept in row-major order (cv2 skips zero-weight entries): na
 *                  source cells, nb sink cells, each <= cap_cells <= SQ_EMD_MAX_CELLS.  The ground distance of two cells is
 *                  sqrt((double)(dx dx + dy dy)) of their integer indices, computed on the fly (no n x m matrix).
 *                  Successive shortest augmenting paths: duals u = 0, v_j = min_i c_ij; Dijkstra from a source with supply
 *                  left over the sink columns, sq_emd_column_chunk() columns per pass of the workgroup, the columns'
 *                  labels, duals and arc lists' heads and the rows' duals in LDS -- relax every column from the newly scanned rows, argmin
 *                  over the unfinalised columns (lowest index on ties), follow that column's flow arcs back to unscanned
 *                  rows; stop at the first column with demand left, add D - dist to the potentials, augment by the
 *                  minimum of the remaining supply, the remaining demand and the backward flows of the path.
 *                  Bounded work: at most max_aug augmentations (0: SQ_EMD_DEFAULT_AUGMENTATIONS (na + nb)) and arc_cap live arcs; reaching either
 *                  ends THAT problem with its status, and the entry's caller reads the text from sq_emd_status_text.
 *                  Outputs per problem (row strides cap_cells / arc_cap): value f64 (:88-89's norm is the caller's);
 *                  status int32 (SQ_EMD_OK, or the first bound met); counts int32 [P, 8] = (na, nb, augmentations, arc
 *                  slots used, search steps, 0, 0, 0 -- all eight written by the kernel); cell_a, cell_b int32 (the kept cells' row-major indices x W + y); w_a, w_b f64 weights;
 *                  u, v f64 duals; arc_i, arc_j int32 and arc_f f64: slot s holds a flow arc (source i, sink j, flow) if
 *                  arc_f > 0 and is free if 0.0.  u_i + v_j <= c_ij for all pairs, equality on the arcs, and
 *                  value = sum flow c = u . w_a + v . w_b, all up to f64 rounding.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_EMD_MAX_CELLS 4096          /* positive cells per map */
#define SQ_EMD_MAX_DIM 16384           /* grid extent (a cell's coordinates pack into 2 x 16 bits with room) */
#define SQ_EMD_MAX_GRID_CELLS 16777216 /* H x W of one dense grid */
#define SQ_EMD_MAX_PROBLEMS 65536
#define SQ_EMD_DEFAULT_AUGMENTATIONS 256 /* x (na + nb): the default cap on augmentations of one problem */
#define SQ_EMD_MAX_ARCS 16384          /* arc slots per problem: 2 (na + nb) at the cell limit */
#define SQ_EMD_OK 0
#define SQ_EMD_TOO_MANY_CELLS 1        /* a map has more than cap_cells cells of positive weight */
#define SQ_EMD_AUGMENTATION_CAP 2      /* max_aug augmentations made and supply is left */
#define SQ_EMD_ARC_CAP 3               /* the flow needs more than arc_cap arcs */
#define SQ_EMD_BAD_GRID 4              /* an extent outside 0..SQ_EMD_MAX_DIM, H W > cells, or a negative / non-finite sum */
#define SQ_EMD_NO_PATH 5               /* a search ended without reaching demand (not reachable with finite weights) */
int sq_emd_column_chunk(void);
const char* sq_emd_status_text(int status);
/* status_host: the P statuses copied to the HOST.  SQ_OK if all are SQ_EMD_OK; otherwise SQ_ERR_UNSUPPORTED, and
 * sq_last_error names the first problem that is not and says why. */
int sq_emd_status_check(const int32_t* status_host, int P);
size_t sq_emd_fill_workspace_bytes(int P, int cells);
int sq_emd_fill(const double* a, int lda, const int32_t* cols_a, const double* b, int ldb, const int32_t* cols_b, int n,
                const int32_t* xtf, const int32_t* ytf, int P, int nan_absent, int grid_h, int grid_w, int cells, double* grids,
                int32_t* dims, uint8_t* flag, void* workspace, size_t workspace_bytes, sq_stream_t stream);
size_t sq_emd_workspace_bytes(int P, int cap_cells, int arc_cap);
int sq_emd_solve(const double* grids, int cells, const int32_t* dims, int P, int cap_cells, int arc_cap, int max_aug,
                 double* value, int32_t* status, int32_t* counts, int32_t* cell_a, double* w_a, int32_t* cell_b, double* w_b,
                 double* u, double* v, int32_t* arc_i, int32_t* arc_j, double* arc_f, void* workspace, size_t workspace_bytes,
                 sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Spot normalisation: the first lines of spatial_vis/get_emd.py (get_emd.py:148-155) -- sc.pp.normalize_total,
 * sc.pp.log1p and sc.pp.scale of the raw spot matrix, then adata[:, gene].X -- restated in f64 (scanpy works in the
 * matrix's own dtype, usually float32: NO digit-for-digit claim against it is made).  X is [n_spots, n_genes] in CSR:
 * indptr int64 [n_spots + 1] and indices int32 [nnz] on the device, data [nnz] f32 (data_kind = SQ_SN_DATA_F32), f64
 * (SQ_SN_DATA_F64) or int32 (SQ_SN_DATA_I32), widened to f64 first; a row's indices strictly increasing, values
 * non-negative and finite.  Every argument is checked before the first launch; the calls are asynchronous on `stream`
 * and never synchronise; no floating-point atomics, every sum in a fixed order that depends only on the shapes: two
 * calls give the same bytes.  1 <= n_spots <= SQ_GT_MAX_SPOTS, 1 <= n_genes <= SQ_SN_MAX_GENES, 0 <= nnz <= SQ_SN_MAX_NNZ.
 * A row whose indptr pair is not 0 <= start <= end <= nnz is read nowhere by any entry.
 *
 *   sq_spot_counts      : c_i = sum_j X_ij (get_emd.py:148-155, normalize_total's counts per cell): counts f64 [n_spots].
 *                         One wave per row, the lanes stride the row's entries with an f64 partial each, the 64 partials
 *                         are combined by a fixed xor butterfly (rows hold 0..n_genes entries).  With integer counts
 *                         and row totals below 2^53 every order is exact: c equals numpy's sum bit for bit; for
 *                         fractional data it is within the any-order bound.  status, one int32 on the device, is set
 *                         to 0 first and then gets SQ_SN_BAD_ORDER (a row's indices not strictly increasing),
 *                         SQ_SN_BAD_INDEX (an index outside [0, n_genes)), SQ_SN_BAD_VALUE (a negative or non-finite
 *                         value) and SQ_SN_BAD_INDPTR (a row's start and end not 0 <= start <= end <= nnz) or-ed in
 *                         (an integer atomic); with a non-zero status no result is to be used.
 *   sq_spot_target      : get_emd.py:148-155, normalize_total's target: after [1] f64 = np.median(c[c > 0]) -- the middle
 *                         value, or (a + b) / 2.0 of the two middle ones -- and n_positive [1] int32 = #(c > 0); no
 *                         positive spot: after = NaN.  Exact for any spot count: the counts are sorted in chunks of
 *                         sq_map_rank_chunk_rows() by the percentile's kernel (csrc/colsort.hip), then the k-th smallest
 *                         is selected by bisection on the f64 bit pattern, counting keys <= x with the upper-bound search
 *                         of csrc/colsort.h over the chunks.  One workgroup.
 *   sq_spot_log_columns : get_emd.py:148-155, normalize_total's division, log1p and adata[:, gene]: L f64 [n_spots, C],
 *                         L[i][c] = log1p(X[i][g] / s_i), g = cols[c] (any order, repeats allowed; NULL: all genes,
 *                         C = n_genes), s_i = (c_i + (c_i == 0)) / after -- scanpy's two divisions in scanpy's
 *                         order; counts and after are device pointers (the outputs of the two entries above).  An
 *                         absent entry gives exactly 0.0.  With a column list: a binary search in the row's sorted
 *                         indices, one thread per (row, column), consecutive threads on consecutive columns; with NULL:
 *                         L is zero-filled and every row scatters its entries (one wave per row).  The two paths give
 *                         the same bytes for the same columns.  log1p is the device library's f64 log1p: L lies
 *                         within 1 ulp of the extended-precision truth rounded to f64 (measured on an MI355X over the
 *                         tests' inputs, largest distance 1.00 ulp: profiles/spot_norm_rate.txt; the tests allow 2).
 *                         n_spots C <= SQ_SN_MAX_CELLS.
 *   sq_spot_scale       : get_emd.py:148-155, sc.pp.scale (zero-centred, max_value=None): per column of L f64 [n, ld],
 *                         mean[c] = sum_i L_ic / n, sd[c] = sqrt(sum_i (L_ic - mean)^2 / (n - 1)) (two-pass), an sd of 0
 *                         becomes 1; write_z = 1: L_ic = (L_ic - mean) / sd in place (a third pass).  Sums run over
 *                         all n rows, zeros included.  2 <= n <= SQ_GT_MAX_SPOTS, 1 <= C <= ld.  16 consecutive columns
 *                         per workgroup (coalesced row reads), 16 row lanes per column that each add every 16th row in
 *                         row order, and an LDS tree in fixed order.  A column that is constant and non-zero gets a
 *                         rounding-noise sd and z (as in scanpy); an all-zero column gives z = 0 exactly.
 *   sq_spot_target_workspace_bytes returns 0 exactly for the refused n_spots (the invariant under "Map statistics").
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_SN_MAX_GENES 1048576
#define SQ_SN_MAX_NNZ 2147483647
#define SQ_SN_MAX_CELLS 1073741824     /* n_spots x C of one L table (8 GiB of f64) */
#define SQ_SN_DATA_F32 0
#define SQ_SN_DATA_F64 1
#define SQ_SN_DATA_I32 2
#define SQ_SN_BAD_ORDER 1
#define SQ_SN_BAD_INDEX 2
#define SQ_SN_BAD_VALUE 4
#define SQ_SN_BAD_INDPTR 8
int sq_spot_counts(const void* data, int data_kind, const int32_t* indices, const int64_t* indptr, int n_spots, int n_genes,
                   long long nnz, double* counts, int32_t* status, sq_stream_t stream);
size_t sq_spot_target_workspace_bytes(int n_spots);
int sq_spot_target(const double* counts, int n_spots, double* after, int32_t* n_positive, void* workspace,
                   size_t workspace_bytes, sq_stream_t stream);
int sq_spot_log_columns(const void* data, int data_kind, const int32_t* indices, const int64_t* indptr, int n_spots,
                        int n_genes, long long nnz, const double* counts, const double* after, const int32_t* cols, int C,
                        double* L, sq_stream_t stream);
int sq_spot_scale(double* L, int n, int ld, int C, double* mean, double* sd, int write_z, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Test and probe hooks (not a stable interface): the switches and bare kernel launches the tests and tools/ use.
 *   sq_dbg_set       : experiment knobs of the GEMM engines (csrc/gemm.hip lists the keys).
 *   sq_dbg_chain_x3  : one launch of the split-mode expand / reduce chain of the 56 x 56 stage (csrc/chain_x3.hip).
 *   sq_dbg_chain_x3w : one launch of the same chain for the 28 x 28 and 14 x 14 stages (csrc/chain_x3w.hip).
 *   sq_dbg_uni_attn  : the attention core of one UNI block, softmax(q k^T / 8) v per (image, head), through the launch the
 *                      forward pass uses (csrc/uni.hip).  qkv [n_images * n_tokens, 3 * heads * 64] -> o [n_images * n_tokens,
 *                      heads * 64], row-major, in `dtype`: SQ_DTYPE_F32 or SQ_DTYPE_BF16; SQ_DTYPE_F16X3: the fp16 hi plane
 *                      followed by the lo plane, n_images * n_tokens * 3 * heads * 64 elements apart in qkv and
 *                      n_images * n_tokens * heads * 64 in o.  1 <= n_tokens <= 256; 16-byte aligned pointers.
 *   sq_dbg_resnet50_taps : sq_resnet50_extract_hw (same arguments, same admitted shapes, same forward and routes) that also
 *                      copies intermediate tensors out as fp32 NHWC: fp32 as is, bf16 widened, split modes hi + lo added in fp32.
 *                      Tap order (SQ_RESNET50_TAPS - 1 = 33 tensors, one after another in `taps`):
 *                        0            the stem's output behind the max-pool, [n, ceil(H/4), ceil(W/4), 64];
 *                        1 + 2k       t1 of bottleneck k (k = 0..15 over layers 1-4 of 3, 4, 6, 3 blocks): the reduce 1x1's output
 *                                     as that block's 3x3 reads it, [n, h, w, planes] on the block's INPUT map (h x w: ceil(H/4) x
 *                                     ceil(W/4) in layer 1; the first block of layers 2-4 still has the previous layer's map),
 *                                     planes = 64, 128, 256, 512 per layer -- whichever launch produced it (its own GEMM, the stem
 *                                     launch, or the previous block's fused tail / chain);
 *                        2 + 2k       y of bottleneck k, the block's output, [n, oh, ow, 4 * planes] (oh x ow: ceil of half the
 *                                     input map in the first block of layers 2-4, else the input map).
 *                      tap_offsets: host array of SQ_RESNET50_TAPS int64: element i = first float of tap i, element 33 = the total.
 *                      taps == NULL: only tap_offsets is filled (to size the buffer), nothing is launched and the other pointers
 *                      may be NULL.  A taps_floats below the total, or a shape sq_resnet50_extract_hw refuses, is an error
 *                      before anything is launched.  t2 and the downsample tensor are not tapped: on the fused routes they
 *                      never leave the CU.
 *   sq_dbg_kmeans_lloyd : sq_kmeans_fit (same bounds, same centring and tolerance, same Lloyd loop, final E-step and cluster
 *                      means) without the k-means++ seeding and the centre gather: the loop starts from init_centers f32
 *                      [n_slides, n_clusters, dim] in CENTRED coordinates (X minus its fp32 column mean), so the tests can put
 *                      centres where no data lies and reach the empty-cluster relocation.  final_centers f32 [n_slides,
 *                      n_clusters, dim] (may be NULL) receives the centres of the last update, centred as well (max_iter = 0:
 *                      init_centers).  large_lists != 0 builds the member lists with the counting sort of sq_kmeans_fit_large
 *                      (n_slides must be 1) on the same slide.  Workspace: sq_kmeans_workspace_bytes.  Writes no seed indices.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_RESNET50_TAPS 34
int sq_dbg_set(int key, int value);
int sq_dbg_chain_x3(int f16, int n2, int ds, int tail, long long P, int W, void* act, void* wts, void* fp, void* frag, void* stream);
int sq_dbg_chain_x3w(int f16, int c, int n2, long long P, const void* t2_hi, const void* t2_lo, const void* res_hi, const void* res_lo,
                     void* y_hi, void* y_lo, void* t1n_hi, void* t1n_lo, const void* w3_hi, const void* w3_lo,
                     const void* w1n_hi, const void* w1n_lo, const float* b3, const float* cs3, const float* b1n, const float* cs1n,
                     int w_tiled, void* stream);
int sq_dbg_uni_attn(int dtype, const void* qkv, void* o, int n_images, int n_tokens, int heads, void* stream);
int sq_dbg_resnet50_taps(int dtype, const void* weights, const float* bias, const uint8_t* patches_u8,
                         const float* patches_f32_nchw, int n_patches, int height, int width, float* features,
                         void* workspace, size_t workspace_bytes, uint32_t* nonfinite_flag, sq_stream_t stream,
                         float* taps, size_t taps_floats, int64_t* tap_offsets);
int sq_dbg_kmeans_lloyd(const float* X, int n_slides, int n_samples, int dim, int n_clusters, const float* init_centers,
                        int large_lists, int max_iter, double tol, int32_t* labels, float* cluster_features, float* final_centers,
                        int32_t* n_iter, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * JPEG tiles: the tiles of a JPEG-compressed tiled TIFF / Aperio SVS level decoded and composed into RGBA regions on the
 * device.  Replaces the host decoding behind the region reads of pre_processing/patch_gen_hdf5.py (slide.read_region at
 * :45 and :108, through OpenSlide) and of spatial_vis/visualize.py:58-66,173; sequoia-pub_amd/wsi/ (TiffSlide, jpeg.py) is the
 * caller.  Every output byte is libjpeg's (baseline Huffman, "islow" IDCT, "fancy" upsampling, the 16-bit fixed-point
 * YCbCr -> RGB), integer throughout; sequoia-pub_amd/csrc/jpeg_core.h holds the arithmetic as host-and-device functions:
 *   entropy     interleaved scan in MCU order; FF 00 -> FF; EXTEND(v, s) = v if v >= 2^(s-1) else v - 2^s + 1; AC symbol rs:
 *               r = rs >> 4, s = rs & 15; s == 0: r == 15 skips 16 coefficients, else end of block; otherwise skip r and read
 *               one coefficient at the zigzag position.  Restart interval Ri: before MCU n > 0 with n % Ri == 0 the partial
 *               byte goes, FF D0+((n / Ri - 1) & 7) is expected and the DC predictors are reset.  Quantisation tables are in
 *               zigzag order; dequantisation is the plain product.
 *   IDCT        13-bit constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172; columns first with a
 *               descale of 11 bits, then rows with 18, each (v + (1 << (n - 1))) >> n; then clamp(v + 128, 0, 255).  libjpeg's
 *               range table wraps rather than clamps for |v| beyond about 512; no encoder of 8-bit images produces that.
 *   upsampling  chroma 2 x 1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, the end
 *               samples copied; 2 x 2: cs[i] = 3 near[i] + far[i] (far row r - 1 for output row 2r, r + 1 for 2r + 1,
 *               replicated at the tile's edge), out[2i] = (3 cs[i] + cs[i-1] + 8) >> 4, out[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4,
 *               first column (4 cs[0] + 8) >> 4, last (4 cs[n-1] + 7) >> 4.  Per tile image: edges replicate inside the tile.
 *   colour      transform != 0 (TIFF photometric 6): cb -= 128, cr -= 128, R = y + ((91881 cr + 32768) >> 16),
 *               G = y + ((-22554 cb - 46802 cr + 32768) >> 16), B = y + ((116130 cb + 32768) >> 16), clamped; 0: as stored.
 * Frames: three components, 8 bits, luma sampling hs x vs in {1 x 1, 2 x 1, 2 x 2} over chroma 1 x 1, extents multiples of
 * 16 in 16..SQ_JPEG_MAX_TILE, the same for every tile of a call.
 *
 * Device inputs of sq_jpeg_decode_tiles (the caller uploads them; all are re-checked on the device, where they live):
 *   scans        the entropy-coded bytes of the tiles, base 16-byte aligned, scans_bytes a multiple of 16 (a lane fetches 16
 *                bytes at a time); a tile's scan may start at any byte.
 *   tile_table   int32 [n_tiles][SQ_JPEG_TILE_WORDS]: scan offset, scan length (bytes of `scans`), table set, restart
 *                interval in MCUs (0: none), selectors (component c at bits 4c: quantisation table in 2 bits, DC table in
 *                1 bit, AC table in 1 bit), three zeros.  Lanes of a wave run as long as the longest scan among them: order
 *                the tiles by scan length.  Up to SQ_JPEG_WAVE_PER_TILE_MAX tiles every tile has a wave to itself (a scan is serial and a wave executes the union
 *                of its lanes' paths); above, 2 to 64 tiles share one.
 *   table_sets   uint8 [n_table_sets][SQ_JPEG_TABLE_SET_BYTES]: four quantisation tables of 64 little-endian uint16 in
 *                zigzag order, then the Huffman tables DC0, DC1, AC0, AC1, each 16 counts and 256 symbols.
 * Outputs: planes uint8 [n_tiles][sq_jpeg_planes_bytes(1, ...)] (Y [tile_h][tile_w], then Cb and Cr [tile_h / vs][tile_w / hs])
 * and status int32 [n_tiles]: SQ_JPEG_OK or why the tile's lane stopped -- a table set index outside the block or a Huffman
 * table whose counts do not make a prefix code or name more than 256 symbols (SQ_JPEG_BAD_TABLE), a scan range outside
 * `scans` or empty or a restart interval or selector word out of range (SQ_JPEG_BAD_RANGE), a scan that ends before its last
 * MCU (SQ_JPEG_TRUNCATED), a code that matches no table entry (SQ_JPEG_BAD_CODE), a run past coefficient 63
 * (SQ_JPEG_BAD_COEF), a missing or wrong restart marker (SQ_JPEG_BAD_RESTART).  A failing tile touches no other tile; its
 * planes hold what was decoded before the stop.  Nothing is read outside the buffers whatever they contain.
 *
 *   sq_jpeg_workspace_bytes : workspace of sq_jpeg_decode_tiles (derived Huffman tables and int16 coefficients); 0 (and an
 *                          sq_last_error message) for a frame outside the above or n_tiles, n_table_sets < 1.
 *   sq_jpeg_planes_bytes : bytes of `planes` for n_tiles tiles; 0 likewise.
 *   sq_jpeg_decode_tiles : three launches (table derivation, entropy decode with one lane per tile and the look-ahead tables
 *                          in LDS, IDCT through LDS with one thread per column and then per row) and one memset, all on `stream`.
 *   sq_jpeg_compose_regions : planes of n_slots tiles -> rgba uint8 [k][h][w][4], the layout sq_patch_filter_px,
 *                          sq_slide_mask_px, sq_resize_u8_gather and sq_pack_rgb_gather take.  regions int32 [k][2]: x, y of
 *                          each region's corner in level pixels (may be negative); tile_slot int32 [tiles_y][tiles_x]: the
 *                          slot in `planes` of each tile of the level, or -1.  A pixel outside 0..level_w-1 x 0..level_h-1, or
 *                          on a tile without a slot (or with a slot outside 0..n_slots-1), is (0, 0, 0, 0); every other has
 *                          alpha 255.  Four adjacent pixels per thread, one 16-byte store where w is a multiple of 4.
 * Entries check scalars and sizes before launching (SQ_ERR_ARG / SQ_ERR_WORKSPACE); they allocate nothing and do not wait.
 *
 * JPEG tiles, split entropy decode (opt-in): sq_jpeg_decode_tiles_split is sq_jpeg_decode_tiles with the entropy launch
 * replaced by one that puts the 64 lanes of a wave on ONE tile's scan (one wave per tile, grid = n_tiles).  Contract: planes
 * and statuses are those of sq_jpeg_decode_tiles, byte for byte, for every input whatever it contains; the same device
 * inputs, outputs, argument checks and error codes; nothing is read outside the buffers.
 *   method      a baseline Huffman scan is self-synchronising (Klein & Wiseman; Weissenberger & Schmidt): a decoder started at
 *               a wrong bit falls into step after a few symbols.  The scan is cut into subsequences of sub_bytes raw bytes
 *               counted from its first byte (stuffed FF 00 pairs count as two), taken 64 at a time; lane 0 of such a round
 *               starts from the confirmed state (the scan's start, or the round before), every other lane at its
 *               subsequence's first bit as if an MCU began there.  Each lane decodes the symbols whose first bit lies in its
 *               subsequence and records where the next one starts (byte, bit, block within the MCU, zigzag index), the block
 *               ends it passed and the sums of the DC differences.  Then lane i + 1 takes lane i's end as its start and
 *               decodes again until a wave vote finds no start changed: lane 0 is exact, so lanes <= r are exact after round r
 *               and the loop ends after at most 63 rounds; every symbol consumes a bit and every lane stops at its
 *               subsequence's end, so it cannot run on.  Exclusive wave scans give each lane the scan-order number of its
 *               first block and its three DC predictors (sums kept in 32 bits: truncation to int16 commutes with addition),
 *               and a last pass from the exact states stores the non-zero coefficients.
 *   fallback    anything irregular -- a state that stays invalid after synchronisation in front of the scan's last block, an
 *               error in the storing pass, a block count other than the frame's, a scan that ends short, a round of 64
 *               subsequences that ends where it began (a marker in a scan without restart interval) -- and the wave
 *               zeroes the tile's coefficients again and lane 0 runs the serial scan of sq_jpeg_decode_tiles on the tile,
 *               which gives the tile's exact status and exact partial coefficients.
 *   restart     tiles with a restart interval > 0 take that serial scan on lane 0 directly (a marker stops the bit reader;
 *               Aperio tiles carry none).
 *   sub_bytes   a multiple of 4 in SQ_JPEG_SPLIT_SUB_MIN..SQ_JPEG_SPLIT_SUB_MAX, or 0 for SQ_JPEG_SPLIT_SUB_DEFAULT; anything
 *               else is SQ_ERR_ARG, the message naming the value.  Scans of any length work with any sub_bytes.
 *   sq_jpeg_split_workspace_bytes : workspace of sq_jpeg_decode_tiles_split (that of sq_jpeg_decode_tiles; lane states live
 *               in registers).  Table derivation, the memset and the IDCT launch are those of sq_jpeg_decode_tiles.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_JPEG_SPLIT_SUB_MIN 16
#define SQ_JPEG_SPLIT_SUB_MAX 256
#define SQ_JPEG_SPLIT_SUB_DEFAULT 128
#define SQ_JPEG_MAX_TILE 1024
#define SQ_JPEG_TILE_WORDS 8
#define SQ_JPEG_TABLE_SET_BYTES 1600
#define SQ_JPEG_MAX_REGION 32768
#define SQ_JPEG_WAVE_PER_TILE_MAX 4096 /* up to this many tiles each has a wave to itself; above, 2 to 64 share one */
#define SQ_JPEG_OK 0
#define SQ_JPEG_BAD_TABLE 1
#define SQ_JPEG_BAD_RANGE 2
#define SQ_JPEG_TRUNCATED 3
#define SQ_JPEG_BAD_CODE 4
#define SQ_JPEG_BAD_COEF 5
#define SQ_JPEG_BAD_RESTART 6
size_t sq_jpeg_workspace_bytes(int n_tiles, int n_table_sets, int tile_w, int tile_h, int hs, int vs);
size_t sq_jpeg_planes_bytes(int n_tiles, int tile_w, int tile_h, int hs, int vs);
int sq_jpeg_decode_tiles(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles, const uint8_t* table_sets,
                         int n_table_sets, int tile_w, int tile_h, int hs, int vs, uint8_t* planes, int32_t* status,
                         void* workspace, size_t workspace_bytes, sq_stream_t stream);
size_t sq_jpeg_split_workspace_bytes(int n_tiles, int n_table_sets, int tile_w, int tile_h, int hs, int vs);
int sq_jpeg_decode_tiles_split(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles,
                               const uint8_t* table_sets, int n_table_sets, int tile_w, int tile_h, int hs, int vs, uint8_t* planes,
                               int32_t* status, void* workspace, size_t workspace_bytes, int sub_bytes, sq_stream_t stream);
int sq_jpeg_compose_regions(const uint8_t* planes, int n_slots, int tile_w, int tile_h, int hs, int vs, int transform,
                            const int32_t* tile_slot, int tiles_x, int tiles_y, int level_w, int level_h, const int32_t* regions,
                            int k, int h, int w, uint8_t* rgba, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * JPEG 2000 tiles: the tiles of an Aperio SVS level with compression 33003 (YCbCr) or 33005 (RGB), each one raw codestream
 * of one tile, decoded into the planes sq_jpeg_compose_regions reads with hs = vs = 1 (three full-resolution uint8 planes
 * per tile, sq_jpeg_planes_bytes(n, tile_w, tile_h, 1, 1)); sequoia-pub_amd/wsi/j2k.py is the caller and parses the marker
 * segments, the library parses the packets.  sequoia-pub_amd/csrc/j2k_core.h holds the arithmetic as host-and-device functions:
 *   packets     LRCP, RLCP, and RPCL / PCRL / CPRL with one precinct per resolution; per packet one non-empty bit, then per
 *               band (LL; HL, LH, HH) and code-block in raster order inclusion (tag tree against layer + 1, later one bit),
 *               missing bit-planes (tag tree, first inclusion), the pass count (0 -> 1, 10 -> 2, 11xx -> 3 + xx,
 *               1111xxxxx -> 6 + x, 111111111xxxxxxx -> 37 + x), Lblock increments (ones up to a zero, Lblock starts at 3) and a
 *               length of Lblock + floor(log2 passes) bits; a byte after FF carries 7 bits; the header ends byte aligned (a
 *               byte more after FF).  The bytes of a block over all layers are one run: gathered when there are several layers.
 *   blocks      MQ decoder of 47 states, 19 contexts (zero coding 0..8, sign 9..13, refinement 14..16, run length 17, uniform
 *               18; initial states 4 for context 0, 3 for 17, 46 for 18, else 0); past the end of its bytes a block reads FF.
 *               Cleanup pass first, then significance, refinement, cleanup per bit-plane over stripes of four rows.
 *               The value is kept doubled with the half of the last decoded plane in it: 3 << p when a sample becomes
 *               significant in plane p, then +- (1 << p) per refinement bit.  Reversible: value >> 1 (towards zero);
 *               irreversible: value * 0.5 * (1 + mantissa / 2048) * 2^(8 + gain - exponent), gain 0 (LL), 1 (HL, LH), 2 (HH).
 *               Bit-planes of a band: guard + exponent - 1, at most SQ_J2K_MAX_PLANES.
 *   wavelet     per component, resolution by resolution, rows then columns, low samples at even positions, borders mirrored
 *               (x[-1] = x[1], x[n] = x[n-2]), an extent of 1 copied.  5/3: x[2n] -= (x[2n-1] + x[2n+1] + 2) >> 2, then
 *               x[2n+1] += (x[2n] + x[2n+2]) >> 1.  9/7 in float32, every product and sum rounded on its own: low * 1.230174105,
 *               high * (1 / 1.230174105), then x[2n] -= 0.443506852 (x[2n-1] + x[2n+1]), x[2n+1] -= 0.882911075 (..),
 *               x[2n] -= -0.052980118 (..), x[2n+1] -= -1.586134342 (..).
 *   components  reversible transform: G = Y - ((Cb + Cr) >> 2), R = Cr + G, B = Cb + G; irreversible: R = Y + 1.402 Cr,
 *               G = Y - 0.34413 Cb - 0.71414 Cr, B = Y + 1.772 Cb; float values round to nearest even; + 128, clamped.
 *               Chroma sampled 2 x 1 is replicated, c[x >> 1].
 * Device inputs of sq_j2k_decode_tiles (re-checked on the device):
 *   streams      the packet bytes of the tiles (what follows SOD), streams_bytes a multiple of 16.
 *   tile_table   int32 [n_tiles][SQ_J2K_TILE_WORDS]: offset, length (bytes of `streams`), parameter set, zero.
 *   param_sets   uint8 [n_param_sets][SQ_J2K_PARAM_BYTES], little-endian int32 words: 0 SQ_J2K_PARAM_MAGIC, 1 chroma column
 *                sampling (1, 2), 2 decomposition levels (0..8), 3 wavelet (1: 5/3 reversible, 0: 9/7), 4 component transform,
 *                5 layers (1..32), 6 progression (0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL), 7 and 8 code-block exponents (2..6),
 *                9..17 precinct exponents of resolutions 0..8 (x | y << 4), then per component 52 words from 18: guard bits,
 *                quantisation style (0 none, 1 derived, 2 expounded), and (exponent, mantissa) of 25 bands (LL, then HL, LH, HH
 *                of resolutions 1..8; a derived style comes expanded).
 * sq_j2k_layout (host pointers, no device) gives the code-blocks, tag-tree nodes and precinct-bands of a parameter set for a
 * tile extent as counts[3]; the maxima over a call's sets size the workspace, and a tile whose set needs more stops with
 * SQ_J2K_BAD_PARAM.  status int32 [n_tiles]: SQ_J2K_OK, SQ_J2K_BAD_PARAM (a field of the set out of range, or the set index),
 * SQ_J2K_BAD_RANGE (offset, length outside `streams`), SQ_J2K_TRUNCATED_HEADER (a packet header runs past the end),
 * SQ_J2K_BAD_LENGTH (missing bit-planes, a pass count or a length that does not fit the band's bit-planes or the stream),
 * SQ_J2K_TRUNCATED_BODY (the lengths of a packet run past the end).  The planes of a failing tile are zero; it touches no
 * other tile.  Every loop is bounded by the stream length, the block area times its bit-planes or the packet count.
 * Four launches (packets: a lane per tile; blocks: a wave per code-block, its samples and flags in LDS; wavelet: a workgroup
 * per tile-component; planes) and a memset on `stream`; entries check before launching, allocate nothing and do not wait.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_J2K_PARAM_BYTES 704
#define SQ_J2K_PARAM_MAGIC 1261587027 /* 'SJ2K' */
#define SQ_J2K_TILE_WORDS 4
#define SQ_J2K_MAX_PLANES 30
#define SQ_J2K_MAX_PRECINCTS 256 /* per resolution of a component */
#define SQ_J2K_OK 0
#define SQ_J2K_BAD_PARAM 1
#define SQ_J2K_BAD_RANGE 2
#define SQ_J2K_TRUNCATED_HEADER 3
#define SQ_J2K_BAD_LENGTH 4
#define SQ_J2K_TRUNCATED_BODY 5
int sq_j2k_layout(const uint8_t* param_set, int tile_w, int tile_h, int32_t* counts);
size_t sq_j2k_workspace_bytes(int n_tiles, int tile_w, int tile_h, int max_blocks, int max_nodes, int max_bands, size_t streams_bytes);
int sq_j2k_decode_tiles(const uint8_t* streams, size_t streams_bytes, const int32_t* tile_table, int n_tiles, const uint8_t* param_sets,
                        int n_param_sets, int tile_w, int tile_h, int max_blocks, int max_nodes, int max_bands, uint8_t* planes,
                        int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * LZW and uncompressed tiles: the tiles of a generic tiled TIFF level with Compression 5 (LZW) or 1 (none), chunky RGB of
 * 8 bits, decoded into the planes sq_jpeg_compose_regions reads with hs = vs = 1 and transform 0 (three full-resolution
 * uint8 planes per tile, R, G, B: sq_jpeg_planes_bytes(n, tile_w, tile_h, 1, 1)); sequoia-pub_amd/wsi/lzw.py is the caller.
 * sequoia-pub_amd/csrc/lzw_core.h holds the code arithmetic, the serial decoder and the status rules as host-and-device
 * functions; every byte is libtiff's.
 *   codes       packed MSB first; behind a Clear (256) code j = 0, 1, ... is 9 bits wide for j < 254, 10 for j < 766, 11 for
 *               j < 1790, then 12 (libtiff's early change), so the bit position of code j is a function of j; the Clear or
 *               EOI (257) that ends a segment is read at the width of its number.  Old-style streams (LSB first, no Clear at
 *               the start) are not read.
 *   entries     code j >= 1 makes entry 257 + j: the string of code j - 1 and the first byte of the string of code j, which
 *               lie next to each other in the output: an entry is (position, length), 8 bytes, and holds no bytes.  A code
 *               above the next free entry is a bad code; one equal to it copies a range that overlaps what it writes.
 *   overrun     as libtiff: entries past 4095 are counted though no code can name them; the data code that would make entry
 *               5119 (the 4863rd behind a Clear) ends the tile with SQ_LZW_TABLE_FULL.  A Clear at any earlier point, after
 *               every code included, restarts the table; consecutive Clears are one.
 *   end         a tile is full after tile_w * tile_h * 3 bytes; a string that runs past that is cut, and bytes behind it
 *               (libtiff's EOI and its slack bits, or anything else) are not read.  A missing EOI is no error.
 *   predictor   2: every byte of a row is the difference to the byte three to its left, modulo 256; undone by a running sum.
 * Device inputs of sq_lzw_decode_tiles (re-checked on the device):
 *   scans        the tile bytes as the file holds them, scans_bytes a multiple of 16; a tile starts 4-byte aligned.
 *   tile_table   int32 [n_tiles][SQ_LZW_TILE_WORDS]: offset, length (bytes of `scans`), zero, zero.
 *   compression  5 or 1; predictor 1 or 2; the same for every tile of a call.
 *   mode         SQ_LZW_MODE_WAVE: the 64 lanes of a wave on one tile -- per round they fetch 64 codes at their computed
 *                positions, a ballot cuts the round at the first Clear, EOI, bad or missing code, the string lengths are
 *                resolved (references into the same round by pointer jumping), a wave prefix sum gives the output positions,
 *                strings whose source lies before the round are copied by all lanes byte-parallel and the others one after
 *                another, each by all lanes (an overlapping range is periodic); the table is in LDS.  SQ_LZW_MODE_LANE: one
 *                lane per tile runs the serial decoder of lzw_core.h with its table in the workspace: the in-library
 *                reference.  Both give the same bytes and statuses for every input.  Compression 1 ignores the mode.
 * Outputs: planes, and status int32 [n_tiles]: SQ_LZW_OK or why the tile stopped -- an offset, length outside `scans` or a
 * length below 1 (SQ_LZW_BAD_RANGE), a stream (or an uncompressed tile) that ends before the tile is full (SQ_LZW_TRUNCATED), a
 * code above the next free entry (SQ_LZW_BAD_CODE), first nine bits that are not the Clear code (SQ_LZW_NO_CLEAR), the table
 * overrun (SQ_LZW_TABLE_FULL), EOI before the tile is full (SQ_LZW_EARLY_EOI).  The planes of a failing tile are zero; it
 * touches no other tile.  Every loop is bounded by the scan length and the tile size.
 *   sq_lzw_workspace_bytes : workspace of sq_lzw_decode_tiles (the chunky bytes of every tile and the lane mode's tables); 0
 *               (and an sq_last_error message) for extents that are no multiples of 16 in 16..SQ_JPEG_MAX_TILE, n_tiles
 *               outside 1..2^20 or a compression other than 1 and 5.
 *   sq_lzw_decode_tiles : two launches on `stream` (decode -- for compression 1 the range check; then unpredict and split
 *               into planes, a wave per row with a wave scan); arguments are checked before the first launch (SQ_ERR_ARG,
 *               SQ_ERR_WORKSPACE); it allocates nothing and does not wait.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_LZW_TILE_WORDS 4
#define SQ_LZW_MODE_WAVE 0
#define SQ_LZW_MODE_LANE 1
#define SQ_LZW_OK 0
#define SQ_LZW_BAD_RANGE 1
#define SQ_LZW_TRUNCATED 2
#define SQ_LZW_BAD_CODE 3
#define SQ_LZW_NO_CLEAR 4
#define SQ_LZW_TABLE_FULL 5
#define SQ_LZW_EARLY_EOI 6
size_t sq_lzw_workspace_bytes(int n_tiles, int tile_w, int tile_h, int compression);
int sq_lzw_decode_tiles(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles, int tile_w, int tile_h,
                        int compression, int predictor, int mode, uint8_t* planes, int32_t* status, void* workspace,
                        size_t workspace_bytes, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident cohort feed: one training or inference batch gathered from tables that stay on the device.
 * It replaces, per batch, what the loader path does on the host: one store open and read per slide
 * (/root/reference/src/read_data.py:38-56), the collate that stacks the readable items (/root/reference/src/utils.py:10-18)
 * and the pinned copy and upload of the loaders of every fold (/root/reference/src/main.py:112-135).  The tables are loaded
 * and uploaded once (sequoia-pub_amd/data.py: CohortTable); ResidentLoader makes the index of every batch.
 *   sq_cohort_gather : x_table f32 [n_slides, row_x] (row_x = tokens * D) and y_table f32 [n_slides, row_y] (row_y = G) ->
 *                      x_out f32 [m, row_x] and y_out f32 [m, row_y], row j of both = row index[j] of the tables, in ONE launch.
 *                      index: int32 [m] in device memory, or null for the identity with m = n_slides.  An index outside
 *                      [0, n_slides) gives all-zero rows (it is compared before it addresses anything).  m = 0 launches
 *                      nothing.  y_table and y_out may both be null: a features-only gather (row_y is then ignored).
 *                      A table whose rows and output rows all start 16-byte aligned (both base pointers on 16 bytes and the
 *                      row a multiple of 4 floats -- decided per call and per table) moves as 16-byte loads and stores per
 *                      lane and then has no tail; any other table moves by the dword.  Every offset is 64-bit; the grid is
 *                      capped at 2048 blocks and strides over the rest.  Asynchronous on `stream`; arguments are checked
 *                      before the launch; no workspace, no atomics, no LDS.
 * ---------------------------------------------------------------------------------------------------------- */
int sq_cohort_gather(const float* x_table, const float* y_table, int n_slides, long long row_x, long long row_y, const int32_t* index,
                     int m, float* x_out, float* y_out, sq_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * CSV text: the spatial prediction table of the reference's spatial_vis/visualize.py:286-304 -- per gene and fold a column,
 * then per gene the fold mean, written with DataFrame.to_csv -- made on the device (sequoia-pub_amd/csvtext.py is the caller).
 *   sq_fold_mean_f32 : out[r, c] = what DataFrame.mean(axis=1) gives for the float32 values x[f * fold_stride + r * ld + c],
 *                      f = 0 .. n_folds - 1 (pandas' nanmean, bit for bit): sum = +0.0; sum += (v is NaN ? +0.0 : v) in fold
 *                      order in fp32; out = sum / (float)count of the values that are not NaN, correctly rounded; count 0 gives
 *                      NaN.  (So -0.0 alone gives +0.0.)  x and out may be columns of one table: out[r * ld_out + c].
 *   sq_csv_format_rows : the bytes DataFrame.to_csv() (default arguments, Linux) writes for rows row_lo .. row_hi - 1 of a
 *                      frame with the int64 index `index` [n], the int64 columns ints [n, n_int] (dense) and the float32
 *                      columns f32 [n, n_f32] (row stride ld_f32), in that column order; the header line is the caller's.
 *                      A row is its cells joined by ',' and ended by '\n'.  int64: plain decimal.  float32: exactly
 *                      numpy.ndarray.astype(str) -- the shortest digits inside the value's rounding interval, the closest
 *                      of them, a tie to the even digit (numpy's Dragon4: a bound counts as inside for an even mantissa only);
 *                      positional for 1e-4 <= |x| < 1e16 with ".0" behind integers ("3333333500000000.0"), else scientific
 *                      with a sign and two exponent digits ("1e-05", "3e+16"); "-0.0", "inf", "-inf"; NaN is the empty cell.
 *                      A cell with its separator is at most SQ_CSV_MAX_CELL_BYTES bytes (csrc/fmt_core.h holds the text of
 *                      a cell as host-and-device functions).
 *                      Outputs: out[0 .. min(total, capacity)), row_offsets int64 [rows + 1] (row i of the call starts at
 *                      row_offsets[i]; the last entry is the total), total int64 [1], status int32 [1]: SQ_CSV_OK, or
 *                      SQ_CSV_OVERFLOW when total > capacity -- then `out` holds part of the text, and no byte at or behind
 *                      `capacity` is ever written.  Three launches in stream order (cell lengths; an exclusive scan of the
 *                      per-workgroup sums by one workgroup; the bytes), the cells of the call dealt as one flat array, so a row
 *                      of 10^5 cells is many workgroups' work and no workgroup waits for another.  Offsets are 64-bit.
 *                      Limits: 1 <= rows, n_int and n_f32 in 0 .. SQ_CSV_MAX_COLUMNS, rows * (1 + n_int + n_f32) <=
 *                      SQ_CSV_MAX_CELLS; out 4-byte aligned.  Asynchronous; arguments are checked before the first launch.
 *   sq_csv_format_workspace_bytes : workspace of sq_csv_format_rows for rows = row_hi - row_lo (one byte per cell plus the
 *                      scan's tables); 0 for shapes outside the limits.
 * ---------------------------------------------------------------------------------------------------------- */
#define SQ_CSV_OK 0
#define SQ_CSV_OVERFLOW 1
#define SQ_CSV_MAX_CELL_BYTES 21
#define SQ_CSV_MAX_COLUMNS 1048576
#define SQ_CSV_MAX_CELLS 1073741824
#define SQ_CSV_MAX_FOLDS 64
int sq_fold_mean_f32(const float* x, int n_folds, long long fold_stride, long long n, int cols, long long ld, float* out, long long ld_out,
                     sq_stream_t stream);
size_t sq_csv_format_workspace_bytes(long long rows, int n_int, int n_f32);
int sq_csv_format_rows(const int64_t* index, const int64_t* ints, int n_int, const float* f32, int n_f32, long long ld_f32,
                       long long row_lo, long long row_hi, uint8_t* out, long long capacity, int64_t* row_offsets, int64_t* total,
                       int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEQUOIA_HIP_H */
