/*
 * mmgnn.h -- C ABI of libmmgnn.so: MI355X (gfx950) kernels for the heterogeneous-GNN
 * message-passing hot path of AdalineL/Multi-Modal-GNN.
 *
 * The reference is pure Python; its "FFI" for this path is the set of ATen / PyG operators
 * that src/model.py dispatches.  Each entry point below names the reference expression it
 * replaces (paths relative to the reference repo).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - extern "C", returns 0 on success, <0 on error (MMG_E_*); the message is available from
 *     mmg_last_error() (thread-local).
 *   - The CALLER owns every buffer: device pointers to contiguous, 16-byte aligned memory.
 *     No allocation, no synchronisation, no global mutable state inside; everything is
 *     enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - Indices are int32 inside (row/col counts are checked to be < 2^31); the edge_index
 *     handed to mmg_csr_build is the reference's int64 [2,E] row-major tensor.
 *   - All features are fp32.  D (feature width) must be 64, 128 or 256.
 *   - Workspace: *_ws_bytes() twins return the scratch size a call needs.
 */
#ifndef MMGNN_H
#define MMGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMG_OK 0
#define MMG_E_ARG (-1)     /* bad argument (shape, null pointer, unsupported D) */
#define MMG_E_LAUNCH (-2)  /* HIP launch / runtime error */
#define MMG_E_WS (-3)      /* workspace too small */

#define MMG_MAX_REL 4      /* relations fused in one aggregate launch */

int mmg_version(void);
const char* mmg_last_error(void);

/* A HIP stream of the library's own (hipStreamNonBlocking, on the current device) -- outside every stream pool of the
 * host framework, so nothing the host code captures into a hipGraph ever lands on it.  The sharded host side
 * (mmgnn/dist.py) issues its EAGER RCCL all-reduces there: torch's process-group watchdog polls the end events of eager
 * collectives with hipEventQuery, and HIP refuses that query -- and invalidates the capture -- while the stream the
 * event was recorded on is capturing (profiles/probes/rccl_event_cache_abort.py). */
int mmg_stream_create(void** stream_out);
int mmg_stream_destroy(void* stream);

/* ---------------------------------------------------------------------------------------
 * CSR construction (consumes the tensors of
 * src/graph_build.py:476-586).  Stable sort of edge ids by edge_index[sort_row]:
 *   rowptr[n_rows+1], col[E] = edge_index[1-sort_row][perm], perm[E] = original edge id.
 * Bit-exact with torch.sort(stable=True) + bincount + cumsum.
 * A key outside [0, n_rows) is never used as an address: it sorts behind the last row and is not counted, so
 * rowptr[n_rows] < n_edges tells the caller that the input was invalid (graph_build.py:618-633 validates up front).
 * ------------------------------------------------------------------------------------- */
size_t mmg_csr_build_ws_bytes(int64_t n_edges, int64_t n_rows);
int mmg_csr_build(const int64_t* edge_index, int64_t n_edges, int64_t n_rows, int sort_row,
                  int32_t* rowptr, int32_t* col, int32_t* perm,
                  void* ws, size_t ws_bytes, void* stream);

/* deg[i] = rowptr[i+1]-rowptr[i]; inv[i] = 1/max(deg,1)  (PyG mean aggregation's clamp;
 * also torch.bincount of src/model.py:297-298 when called on the has_lab CSR) */
int mmg_row_degree(const int32_t* rowptr, int64_t n_rows, int32_t* deg, float* inv_deg, void* stream);
/* in-degree of the column side: cnt[j] = #edges with col == j; inv[j] = 1/max(cnt,1) */
int mmg_col_degree(const int32_t* col, int64_t n_edges, int64_t n_cols, int32_t* cnt, float* inv_cnt,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * Sparse aggregates (replace PyG SAGEConv's gather + scatter-mean, call site
 * src/model.py:125-131,256, and their backward).  All relations share the ROW axis
 * (patients, CSR-by-patient), so up to MMG_MAX_REL relations are fused per launch.
 *
 * gather:   out[i,:] (+)= sum_r  rowscale_r[i] * sum_{k in row_r(i)} table_r[col_r[k], :]
 *           (vocab -> patient forward; patient -> vocab backward)
 * scatter:  out_r[j,:]  = colscale_r[j] * sum_{k: col_r[k]=j} rowscale_r[row(k)] * x[row(k), :]
 *           (patient -> vocab forward; vocab -> patient backward)
 * rowscale / colscale entries may be NULL (= 1).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const int32_t* rowptr;   /* [n_rows+1] */
  const int32_t* col;      /* [E] */
  const float* rowscale;   /* [n_rows] or NULL */
  const float* colscale;   /* [n_cols] or NULL */
  const float* table;      /* gather: [n_cols, D] source rows */
  float* out;              /* scatter: [n_cols, D] destination rows */
  int32_t n_cols;
  uint32_t flags;          /* MMG_REL_SIMPLE: no (row, col) pair occurs twice -- enables the 0/1 indicator
                              (bf16-split MFMA) kernels; multigraphs take the counting fp32 path */
  const uint64_t* mask_t;  /* NULL, or the relation's adjacency as bit planes (mmg_rel_mask_build): word
                              [row / 64][col][(row % 64 / 8) & 1] has bit 16 * (row % 64 / 16) + 4 + row % 8 set
                              iff (row, col) is an edge (four 16-bit fields, one per 16 rows, each holding 8 row
                              bits << 4); [ceil(n_rows / 64)][pad32(n_cols)][2] words.  Simple relations only. */
  const uint16_t* mask_r;  /* NULL, or the same adjacency row-major for the gather: field
                              [row][(col % 16 / 8) & 1][col / 16] = (8 item bits of cols 16 (col/16) + 8 half + 0..7)
                              << 4; [n_rows][2][pad32(n_cols) / 16] uint16. */
} mmg_rel_t;
#define MMG_REL_SIMPLE 1u

/* One-off per static graph: the bit-plane form of a CSR-by-row relation (40 B per patient at the eICU vocab
 * instead of 4 B per edge).  The scatter kernels expand indicator fragments for the matrix cores straight from
 * these words.  mask_t and mask_r must each hold mmg_rel_mask_words(n_rows, n_cols) uint64 (8-byte units for both);
 * they are zeroed here.  Either may be NULL (not built). */
size_t mmg_rel_mask_words(int64_t n_rows, int32_t n_cols);
int mmg_rel_mask_build(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t n_cols,
                       uint64_t* mask_t, uint16_t* mask_r, void* stream);

/* mmg_gather_rows: below, with the producer epilogues */

/* mmg_scatter_rows: out[col] = sum over the edges (row, col) of rowscale[row] * x[row], times colscale[col].
 * Precision.  A launch with a rowscale, a multigraph relation, a relation without bit planes or more than 352 padded items
 * adds the fp32 terms themselves in fp32 (the matrix-core kernels multiply three exact bf16 pieces of each): every output
 * has the accuracy of an fp32 sum against the sum of |terms| of ITS OWN element (6e-7 of it), whatever the magnitudes in x.
 * The forward launch -- no rowscale, every relation MMG_REL_SIMPLE with mask_t, n_rows >= 64 -- multiplies two f16 pieces
 * of x * 2^e, e chosen by each wave for the row range (a few hundred rows) of the 32-column strip that it streams.  With
 * L = the largest finite magnitude among the strip's 32 columns over the rows of that range streamed so far (a 16-row block
 * more than ~2^12 above everything before it is multiplied exactly and does not count):
 *   - a term of at least 2^-15 L is kept to 2^-22 of itself (a block above L: to 2^-22 or exactly); an output whose terms
 *     are all such is within 6e-7 of the sum of its |terms|, as above;
 *   - a smaller term carries an ABSOLUTE error of up to 2^-37 L (2^-25 2^-e, with 2^(13 - e) between L / 4 and 2 L): it
 *     loses a bit per factor of two below 2^-15 L and is lost altogether 2^37 below.  That is the error of an fp32 running
 *     sum where small and large terms enter the same sum, but an output column (or item) whose terms ALL lie that far below
 *     the other columns of its strip, or below earlier rows of the same range, is not kept to fp32 accuracy of itself.
 *     A partial sum more than 2^100 below a later L of the range is unspecified within that absolute error.
 * A caller whose columns differ by more than 2^15 inside a 32-column strip and who needs each to fp32 accuracy passes a
 * rowscale of ones (the exact kernels).  A NaN or an infinity in x[row, c] makes column c of the outputs non-finite (of
 * every item, as in the dense layers) and changes no other column. */
size_t mmg_scatter_rows_ws_bytes(const mmg_rel_t* rels, int n_rel, int64_t n_rows, int D);
int mmg_scatter_rows(const mmg_rel_t* rels, int n_rel, int64_t n_rows, int D,
                     const float* x, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dense layers: fp32 products as an exact six-term bf16 split on the bf16 matrix cores
 * (v_mfma_f32_32x32x16_bf16, fp32 accumulation; 2e-6 of an fp64 reference).  Replace torch.nn.Linear /
 * BatchNorm1d / ReLU / Dropout / F.normalize of src/model.py:93-105,229-232,258-269 and the
 * lin_l / lin_r of SAGEConv.
 *
 * Prologue applied to X on load (all optional):
 *   x' = dropout( relu( x * scale[k] + shift[k] ) )      scale/shift = folded BatchNorm
 * ------------------------------------------------------------------------------------- */
#define MMG_ACT_NONE 0
#define MMG_ACT_RELU 1
#define MMG_ACT_LEAKY_RELU 2
#define MMG_ACT_ELU 3
typedef struct {
  const float* scale;      /* [K] or NULL: no affine */
  const float* shift;      /* [K] */
  int relu;                /* activation after the affine: MMG_ACT_NONE / _RELU / _LEAKY_RELU (slope 0.01) / _ELU (alpha 1)
                              -- the three src/model.py:145-152 accepts.  The dense kernels' prologue takes NONE / RELU
                              only (patient_transform and the heads are ReLU by construction, model.py:93-103,373-386);
                              the materialising / backward kernels (mmg_affine_act_drop*, mmg_bn_bwd_*) take all four. */
  float drop_p;            /* 0 = no dropout */
  uint64_t seed;           /* dropout RNG: keep(seed, site, global_row*K + k) */
  uint32_t site;
  int64_t row_offset;      /* global index of row 0 (patient sharding), >= 0.  The element index (row_offset + row) * K + k
                              is honoured as a full 64-bit number by every kernel that draws a mask; it must stay
                              below 2^63, i.e. (row_offset + M) * K < 2^63 (tested up to 2^51) */
  const uint64_t* seed_ptr;/* optional DEVICE pointer: when non-NULL the seed is read from it at run time
                              (lets a captured hipGraph draw fresh masks on every replay) */
} mmg_prologue_t;

/* Y[M,N] = prologue(X)[M,K] . W[N,K]^T (+ bias[N]) (+ Y if MMG_LIN_ACCUMULATE).
 * MMG_LIN_W_KN: W is stored [K,N] (Y = X . W) -- the data-gradient GEMMs of the backward pass read the forward
 * weight in place instead of a transposed copy. */
#define MMG_LIN_ACCUMULATE 1
#define MMG_LIN_W_KN 2
/* Training-mode BatchNorm1d fold (what mmg_bn_finalize computes from the column sums, training = 1: scale / shift / mean /
 * rstd, running statistics advanced n_updates times) taken in the launch that sums a producer's partial statistics rows.
 * Single-GPU form: a patient-sharded run has to all-reduce the sums first. */
typedef struct {
  int64_t count;
  const float* gamma; const float* beta;      /* [N], nullable: 1 / 0 */
  float* running_mean; float* running_var;    /* [N], nullable: not advanced */
  int n_updates;
  float momentum; float eps;
  float* scale; float* shift; float* mean; float* rstd;   /* [N] outputs; mean / rstd nullable */
} mmg_bn_fin_t;
/* The statistics pass of a BatchNorm backward taken from the kernel that PRODUCES its upstream gradient.
 * mmg_bn_bwd_stats (and _stats2) read the [M, N] upstream gradient and the [M, N] pre-BatchNorm activation once more; a
 * producer that is handed this descriptor sums them from its output tile while it is still in registers and only reads
 * Y.  `sums` receives exactly what mmg_bn_bwd_stats(G = the producer's output, y, pro, mean, rstd) would, summed in a
 * fixed order (16 rows in fp32, the rest in fp64); with accumulate != 0 that is ADDED to `sums` -- the two sums are
 * linear in G, so two producers whose outputs go through the same BatchNorm with their own dropout masks (the two
 * encode_nodes passes of a training step, mmg_bn_bwd_stats2) each add their share.
 * Autograd of  nn.Linear -> BatchNorm1d -> ReLU -> Dropout  chains (src/model.py:93-101, 258-269): the gradient a layer
 * hands down is the upstream gradient of the BatchNorm below it.  Fused (activation none or relu) in:
 *   mmg_linear_fwd                  dX = dY . W  (MMG_LIN_W_KN) of a plain linear, e.g. the heads' first layer; no prologue,
 *                                   no accumulate;  M > 512, N % 128 == 0, K in {64, 128}
 *   mmg_linear_bnbwd                dX;  K = N = 128 without a weight gradient (not MMG_BNBWD_BN2: refused)
 *   mmg_gather_rows                 the final `out` (accumulate or not);  the bit-plane layouts, D >= 128
 * elsewhere the producer is followed by the separate statistics pass: defined for everything the producer accepts. */
typedef struct {
  const float* y;                 /* [M, N] pre-BatchNorm activation of the layer below */
  const mmg_prologue_t* pro;      /* its fold (scale / shift), activation and dropout */
  const float* mean;              /* [N] */
  const float* rstd;              /* [N] */
  double* sums;                   /* [2, N] out (in / out with accumulate) */
  int accumulate;
  void* ws;                       /* >= mmg_epi_ws_bytes(M, N) */
  size_t ws_bytes;
} mmg_next_bn_t;
/* The epilogue of a producer (mmg_linear_fwd, mmg_gather_rows), computed from its output tile in registers instead of a
 * second pass over the output.  epi->mode (epi == NULL: MMG_EPI_NONE):
 *   MMG_EPI_NONE     the producer alone
 *   MMG_EPI_STATS    col_sums [2, N] (fp64) = (sum_m Y, sum_m Y^2) of the FINAL output, the batch statistics of the
 *                    BatchNorm that follows (src/model.py:95,99,258-262); fin (nullable) folds it in the same launch.
 *                    M > 0.  The bf16-split GEMM (M > 512) and the bit-plane gathers sum them in their epilogue; other
 *                    launches are followed by a separate column reduction.
 *   MMG_EPI_NEXT_BN  the statistics of the BatchNorm backward that consumes the output, see mmg_next_bn_t
 *   MMG_EPI_L2       linear only, no flags: the row L2 normalisation of the output (patient_transform's last Linear +
 *                    F.normalize(p=2, dim=1), src/model.py:103,232) in the same kernel: Y = y / max(|y|_2, eps) per row,
 *                    rnorm [M] = 1 / max(|y|_2, eps) (what mmg_l2norm_fwd returns and mmg_l2norm_bwd takes)
 * Fields a mode does not name are ignored; a descriptor with both col_sums and next is refused.  The workspace of STATS
 * and of every mmg_next_bn_t: mmg_epi_ws_bytes(M, N).
 * mmg_linear_fwd_supported: L2 needs M > 512 and N, K in {64, 128}; the other modes take every shape of the plain GEMM
 *   (M >= 0, K in {64, 128, 256}, N a multiple of 64 up to 4096). */
#define MMG_EPI_NONE 0
#define MMG_EPI_STATS 1
#define MMG_EPI_NEXT_BN 2
#define MMG_EPI_L2 3
typedef struct {
  int mode;                       /* MMG_EPI_* */
  double* col_sums;               /* STATS: [2, N] out */
  const mmg_bn_fin_t* fin;        /* STATS: the BatchNorm fold, or NULL */
  void* ws; size_t ws_bytes;      /* STATS */
  const mmg_next_bn_t* next;      /* NEXT_BN */
  float* rnorm; float eps;        /* L2: [M] out, eps */
} mmg_fwd_epi_t;
size_t mmg_epi_ws_bytes(int64_t M, int N);
int mmg_linear_fwd_supported(int mode, int64_t M, int N, int K);
int mmg_linear_fwd(const float* X, const mmg_prologue_t* pro, const float* W, const float* bias, float* Y, int64_t M, int N,
                   int K, int flags, const mmg_fwd_epi_t* epi, void* stream);
/* The same layer under two dropout masks in ONE launch: Y0 = pro0(X) . W^T + b, Y1 = pro1(X) . W^T + b, where pro0 and pro1
 * agree in scale, shift, relu, drop_p (> 0), seed, seed_ptr and row_offset and differ in the site alone (the second linear of
 * the two encode_nodes passes of a training step, src/model.py:294,301).  X is read, folded and split once.  Both epilogues
 * are MMG_EPI_STATS with their own col_sums and workspaces; their folds (both, or neither) are taken in one launch, fin of
 * epi0 before fin of epi1 -- they may advance the same running statistics.  Y0, Y1, the sums and the folds are bit for bit
 * those of two mmg_linear_fwd calls in that order.  mmg_linear_fwd_dual_supported: M > 512, N = K = 128; anything else, and
 * prologues that differ in more than the site, are refused with MMG_E_ARG before anything is launched. */
int mmg_linear_fwd_dual_supported(int64_t M, int N, int K);
int mmg_linear_fwd_dual(const float* X, const mmg_prologue_t* pro0, const mmg_prologue_t* pro1, const float* W,
                        const float* bias, float* Y0, float* Y1, int64_t M, int N, int K, const mmg_fwd_epi_t* epi0,
                        const mmg_fwd_epi_t* epi1, void* stream);
/* A compact second problem on the same W and bias that RIDES in a dense MMG_EPI_L2 launch: the third linear + L2 norm of
 * the two encode_nodes passes of a training step (src/model.py:294,301,103,232).  The first pass only feeds tabular_mlp, so
 * its tail runs on the n_sel low-degree rows alone -- two launches of a few microseconds of work each, alone on the chip.
 * mmg_linear_fwd_rider is, in this order,
 *   mmg_linear_fwd(X, pro, W, bias, Y, M, N, K, 0, epi)                                          the dense launch
 *   mmg_affine_act_drop_rows(X_a, pro_a, rows, n_sel, act_a, K)                                  masks of the ORIGINAL rows
 *   mmg_linear_fwd(act_a, NULL, W_a, bias_a, Y_a, n_sel, N, K, 0, epi_a)
 * in ONE launch, every output bit for bit: the dense launch keeps its grid, its tile-to-workgroup map and its code, and
 * every workgroup goes on over the rider's 32-row tiles in the same round-robin behind its last dense tile.  X_a [M, K] is
 * the tensor the listed rows are read from, pro_a its prologue (all four activations), act_a [n_sel, K] the prologue'd rows
 * (the weight gradient reads them), Y_a [n_sel, N] and epi_a->rnorm [n_sel] the normalised rows and their reciprocal norms.
 * mmg_linear_fwd_rider_supported: M > 512, N = K = 128, and n_sel = 0 (the dense launch alone) or 512 < n_sel <= M (the
 * lists the third call above takes with the L2 epilogue; a shorter list goes to the fp32 kernel of the small tables and an
 * L2 pass, which the caller keeps launching).  Refused with MMG_E_ARG before anything is launched: an unsupported shape, an
 * epilogue other than MMG_EPI_L2 or two different eps, a dense prologue that is absent or the identity, W_a / bias_a other
 * than W / bias, a null buffer, a rider output (act_a, Y_a, rnorm) that overlaps another tensor of the call.  rows: ids in
 * [0, M) (not checked: they are on the device).
 * Probe row: the dense launch's own (MMG_PROBE_LINEAR_FWD, M, N, K, 4 | 32) with the flag 32768; the rider's rows are
 * left out of the pricing. */
int mmg_linear_fwd_rider_supported(int64_t M, int N, int K, int64_t n_sel);
int mmg_linear_fwd_rider(const float* X, const mmg_prologue_t* pro, const float* W, const float* bias, float* Y, int64_t M,
                         int N, int K, const mmg_fwd_epi_t* epi, const float* X_a, const mmg_prologue_t* pro_a,
                         const int64_t* rows, int64_t n_sel, const float* W_a, const float* bias_a, float* act_a, float* Y_a,
                         const mmg_fwd_epi_t* epi_a, void* stream);
int mmg_gather_rows(const mmg_rel_t* rels, int n_rel, int64_t n_rows, int D, float* out, int accumulate,
                    const mmg_fwd_epi_t* epi, void* stream);

/* dW[N,K] (+)= dY[M,N]^T . prologue(X)[M,K]   (reduction over the M rows);
 * dbias (nullable, [N]) (+)= the column sums of dY -- the bias gradient of the same layer, from the same pass */
size_t mmg_linear_wgrad_ws_bytes(int64_t M, int N, int K);
int mmg_linear_wgrad(const float* dY, const float* X, const mmg_prologue_t* pro, float* dW, float* dbias,
                     int64_t M, int N, int K, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* The weight gradient is the fixed-order sum of per-workgroup partial slabs; that sum is a launch of a few microseconds
 * behind every layer.  mmg_linear_wgrad_deferred leaves the slabs in `ws` (which then has to stay untouched) and fills
 * `job`; mmg_wgrad_reduce_group sums the slabs of up to MMG_WGRAD_REDUCE_MAX layers in ONE launch (nobody reads a weight
 * gradient before the optimizer).  Two jobs of one launch must not write the same dW (an accumulating second
 * contribution goes into a later launch); job.slab == NULL (a small-M launch wrote dW directly) is skipped. */
#define MMG_WGRAD_REDUCE_MAX 16
typedef struct {
  const float* slab; int64_t n4; int n_split;     /* n_split slabs of n4 float4 each */
  float* dW; float* dbias; int64_t nk4;           /* float4s [0, nk4) -> dW, the rest -> dbias */
  int accumulate;
} mmg_wgrad_reduce_t;
int mmg_linear_wgrad_deferred(const float* dY, const float* X, const mmg_prologue_t* pro, float* dW, float* dbias,
                              int64_t M, int N, int K, int accumulate, void* ws, size_t ws_bytes, void* stream,
                              mmg_wgrad_reduce_t* job);
int mmg_wgrad_reduce_group(const mmg_wgrad_reduce_t* jobs, int n_jobs, void* stream);
/* 1: a launch of this shape writes / accumulates dW itself (one row range: no slabs) -- an accumulating call of that kind
 * must not overtake a deferred job of the same gradient */
int mmg_linear_wgrad_is_direct(int64_t M, int N, int K);

/* column reductions over rows: out[0,:] = sum_m A[m,:], out[1,:] = sum_m A[m,:]*B[m,:] (fp64 out) */
size_t mmg_col_reduce2_ws_bytes(int64_t M, int N);
int mmg_col_reduce2(const float* A, const float* B, double* out, int64_t M, int N,
                    void* ws, size_t ws_bytes, void* stream);

/* BatchNorm statistics -> folded scale/shift (+ running-stat update, momentum 0.1, unbiased var)
 *   sums[2,N] fp64 = (sum y, sum y^2) over `count` rows (already all-reduced when sharded).
 *   training != 0: mean/var from sums; running_* updated `n_updates` times (F7 double update).
 *   training == 0: scale/shift from running stats.
 *   Outputs: scale[N] = gamma*rstd, shift[N] = beta - mean*scale, mean[N], rstd[N]. */
int mmg_bn_finalize(const double* sums, int64_t count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int training, int n_updates,
                    float momentum, float eps, float* scale, float* shift, float* mean, float* rstd,
                    int N, void* stream);

/* out = dropout(relu(y*scale + shift))  materialised                                */
int mmg_affine_act_drop(const float* Y, const mmg_prologue_t* pro, float* out, int64_t M, int N,
                        void* stream);
/* The same for a subset of rows:  out[s, :] = dropout(relu(y[rows[s], :]*scale + shift)),  s < n_sel, the dropout
 * mask being the one of row rows[s] of the full tensor.  (src/model.py:294 runs encode_nodes a first time only to feed
 * tabular_mlp, which model.py:312-322 applies to the low-degree patients: everything after the last BatchNorm of that
 * pass -- model.py:99-103 -- runs on those rows alone.) */
int mmg_affine_act_drop_rows(const float* Y, const mmg_prologue_t* pro, const int64_t* rows, int64_t n_sel,
                             float* out, int N, void* stream);

/* Backward through dropout -> relu -> affine(BN):
 *   g_out = g * keepmask/(1-p) * [y*scale+shift > 0]
 * pass 1 (stats):  sums[0,:] = sum g_out ; sums[1,:] = sum g_out * xhat,  xhat = (y-mean)*rstd
 * pass 2 (apply):  dy = scale * (g_out - c0[k] - xhat*c1[k]),  c0 = sums0/count, c1 = sums1/count
 *                  (eval mode: sums = NULL, c0 = c1 = 0).  `sums` is the (all-reduced, when sharded) output of pass 1
 *                  and inv_count = 1/count; dbeta / dgamma (nullable, [N] float) receive sums0 / sums1, the gradients
 *                  of the BatchNorm bias / weight.  accumulate != 0: dY += (the two encode_nodes passes of a training
 *                  step share their first layer: the second pass adds its gradient to the first one's). */
int mmg_bn_bwd_stats(const float* G, const float* Y, const mmg_prologue_t* pro, const float* mean,
                     const float* rstd, double* sums, int64_t M, int N, void* ws, size_t ws_bytes,
                     void* stream);
int mmg_bn_bwd_apply(const float* G, const float* Y, const mmg_prologue_t* pro, const float* mean,
                     const float* rstd, const double* sums, double inv_count, float* dbeta, float* dgamma,
                     float* dY, int64_t M, int N, int accumulate, void* stream);

/* Two upstream gradients through the SAME BatchNorm + ReLU, each with its own dropout mask (pro2: only its dropout fields
 * are used) -- the two encode_nodes passes of a training step (src/model.py:294 and :301 -> :251) see the same
 * Linear + BatchNorm1d in front of their first Dropout (model.py:93-96), i.e. they share that layer:
 * g_out = g_out(G; pro) + g_out(G2; pro2), one statistics pass and one apply pass instead of two of each. */
int mmg_bn_bwd_stats2(const float* G, const float* G2, const float* Y, const mmg_prologue_t* pro,
                      const mmg_prologue_t* pro2, const float* mean, const float* rstd, double* sums, int64_t M, int N,
                      void* ws, size_t ws_bytes, void* stream);
int mmg_bn_bwd_apply2(const float* G, const float* G2, const float* Y, const mmg_prologue_t* pro,
                      const mmg_prologue_t* pro2, const float* mean, const float* rstd, const double* sums,
                      double inv_count, float* dbeta, float* dgamma, float* dY, int64_t M, int N, void* stream);

/* The same backward for an upstream gradient that is zero outside a short list of rows (G_rows [n_sel, N] holds the rows
 * rows[s]; masks are those of the ORIGINAL rows):  mmg_bn_bwd_stats_rows gives the sums of pass 1 from the listed rows
 * alone; mmg_bn_bwd_apply with G = NULL writes the dense part of pass 2; mmg_bn_bwd_apply_rows adds scale * g_out to the
 * listed rows of dY (rows must be distinct). */
size_t mmg_bn_bwd_stats_rows_ws_bytes(int N);
int mmg_bn_bwd_stats_rows(const float* G_rows, const float* Y, const int64_t* rows, int64_t n_sel,
                          const mmg_prologue_t* pro, const float* mean, const float* rstd, double* sums, int N,
                          void* ws, size_t ws_bytes, void* stream);
int mmg_bn_bwd_apply_rows(const float* G_rows, const float* Y, const int64_t* rows, int64_t n_sel,
                          const mmg_prologue_t* pro, float* dY, int N, void* stream);

/* The BatchNorm (or L2-norm) backward folded into the data-gradient GEMM of the linear in front of it -- autograd of
 * nn.Linear behind BatchNorm1d + relu + dropout (src/model.py:93-101,258-269) or behind F.normalize.  In ONE pass over the
 * upstream gradient and the activation: dZ [M, K] = that backward, written once for the weight gradient of the layer,
 * and dX [M, N] = dZ . W with W stored [K, N] (the forward weight in place, as MMG_LIN_W_KN).  a->mode:
 *   MMG_BNBWD_BN    pass 2 of mmg_bn_bwd_apply at (G, y): pro, mean, rstd, sums, inv_count, dbeta, dgamma as there (sums
 *                   NULL: eval mode; pro or pro->scale NULL: no BatchNorm, relu / dropout only)
 *   MMG_BNBWD_L2    mmg_l2norm_bwd: dZ = rnorm * (G - y * <G, y>), y = the normalised rows (0 dot product where the norm
 *                   was clamped at eps)
 *   MMG_BNBWD_BN2   mmg_bn_bwd_apply2: G and G2 through the same BatchNorm + relu, pro2 = the dropout of G2
 *   MMG_BNBWD_ROWS  mmg_bn_bwd_apply with G = NULL + mmg_bn_bwd_apply_rows: an upstream gradient that is zero outside a
 *                   list of rows; G [n_sel, K] holds the listed rows back to back (NULL allowed iff n_sel == 0) and
 *                   row_pos [M] the position of a row in that list or -1
 * The BatchNorm modes take relu only.  Fields a mode does not name are ignored.
 * next (nullable; refused with MMG_BNBWD_BN2): the statistics of the BatchNorm backward that consumes dX, see
 *   mmg_next_bn_t.
 * wg (nullable): the weight gradient of the same layer in the same launch -- what
 *   mmg_linear_wgrad_deferred(dZ, X, wg->pro, wg->dW, wg->dbias, M, K, N, wg->accumulate, wg->ws, wg->ws_bytes, ., wg->job)
 *   would compute: dW [K, N] (+)= dZ^T . pro(X), dbias [K] (+)= the column sums of dZ, taken while dZ is still on chip.
 *   The slabs are left in ws and described in *wg->job for mmg_wgrad_reduce_group; job == NULL sums them before
 *   returning.  With wg, dZ may be NULL: it is then not written.  X [M, N] is the layer input; its prologue takes relu
 *   only.
 * mmg_linear_bnbwd_supported: M > 512, and K, N in {64, 128} for BN and L2 without wg; K = N = 128 otherwise. */
#define MMG_BNBWD_BN 0
#define MMG_BNBWD_L2 1
#define MMG_BNBWD_BN2 2
#define MMG_BNBWD_ROWS 3
typedef struct {
  int mode;                       /* MMG_BNBWD_* */
  const float* G;                 /* [M, K] upstream gradient; ROWS: [n_sel, K], the listed rows */
  const float* G2;                /* BN2: [M, K] the second upstream gradient */
  const int32_t* row_pos;         /* ROWS: [M] */
  int64_t n_sel;                  /* ROWS */
  const float* y;                 /* [M, K] BN / BN2 / ROWS: pre-BatchNorm activation; L2: the normalised rows */
  const mmg_prologue_t* pro;      /* BN / BN2 / ROWS: its fold, activation and dropout (BN: may be NULL) */
  const mmg_prologue_t* pro2;     /* BN2: the dropout of G2 (only its dropout fields are used) */
  const float* mean;              /* BN / BN2 / ROWS, with pro->scale: [K] */
  const float* rstd;              /* [K] */
  const double* sums;             /* [2, K] of mmg_bn_bwd_stats, or NULL (eval mode) */
  double inv_count;
  float* dbeta;                   /* [K] or NULL */
  float* dgamma;                  /* [K] or NULL */
  const float* rnorm;             /* L2: [M] */
  float eps;                      /* L2 */
} mmg_bnbwd_t;
typedef struct {
  const float* X;                 /* [M, N] input of the linear */
  const mmg_prologue_t* pro;      /* its prologue (BatchNorm fold, relu, dropout) or NULL */
  float* dW;                      /* [K, N] */
  float* dbias;                   /* [K] or NULL */
  int accumulate;
  void* ws;                       /* >= mmg_linear_bnbwd_wgrad_ws_bytes(M, N, K) */
  size_t ws_bytes;
  mmg_wgrad_reduce_t* job;        /* deferred slab sum, or NULL */
} mmg_bnbwd_wgrad_t;
int mmg_linear_bnbwd_supported(int mode, int64_t M, int N, int K, int with_wgrad);
size_t mmg_linear_bnbwd_wgrad_ws_bytes(int64_t M, int N, int K);
int mmg_linear_bnbwd(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                     const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, void* stream);
/* The backward counterpart of mmg_linear_fwd_rider: the L2 backward + data gradient of the third linear of BOTH
 * encode_nodes passes in one launch.  mmg_linear_bnbwd_rider is, in this order,
 *   mmg_linear_bnbwd(b, W, dZ, dX, M, N, K, next, NULL)                                        b->mode == MMG_BNBWD_L2
 *   mmg_linear_bnbwd(a, W_a, dZ_a, dX_a, n_sel, N, K, NULL, NULL)                              a->mode == MMG_BNBWD_L2
 *   mmg_bn_bwd_stats_rows(dX_a, next_a->y, rows, n_sel, next_a->pro, next_a->mean, next_a->rstd, next_a->sums, N,
 *                         next_a->ws, next_a->ws_bytes)                                        (next_a != NULL)
 * every output bit for bit: the dense launch keeps its grid, tile-to-workgroup map, code and partial statistics (the rider's
 * tiles take no part in the next-BatchNorm epilogue) and every workgroup goes on over the rider's 32-row tiles behind its
 * last dense tile; the statistics pass over the listed rows follows, and ONE launch sums the partial rows of `next` and of
 * the listed rows, each in the order of its own launch.  next_a (nullable) describes the BatchNorm backward that consumes
 * dX_a AT THE LISTED ROWS: y [M, N] the pre-BatchNorm activation those rows belong to, accumulate = 0, ws of at least
 * mmg_bn_bwd_stats_rows_ws_bytes(N) bytes that does not overlap next->ws (both hold partial rows until they are summed).
 * mmg_linear_bnbwd_rider_supported: M > 512, N = K = 128, n_sel = 0 (the dense call alone) or 512 < n_sel <= M (what the
 * second call above accepts).  Refused with MMG_E_ARG before anything is launched: an unsupported shape, a mode other than
 * MMG_BNBWD_L2, W_a other than W, different eps, a null buffer, a rider output (dZ_a, dX_a) that overlaps another tensor of
 * the two problems, overlapping workspaces, and whatever mmg_linear_bnbwd refuses.
 * Probe row: the dense launch's own (MMG_PROBE_LINEAR_FWD, M, N, K, 64 [| 512]) with the flag 32768; the rider's rows are
 * left out of the pricing. */
int mmg_linear_bnbwd_rider_supported(int64_t M, int N, int K, int64_t n_sel);
int mmg_linear_bnbwd_rider(const mmg_bnbwd_t* b, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                           const mmg_next_bn_t* next, const mmg_bnbwd_t* a, const float* W_a, float* dZ_a, float* dX_a,
                           int64_t n_sel, const int64_t* rows, const mmg_next_bn_t* next_a, void* stream);
/* mmg_linear_bnbwd(a, W, dZ, dX, M, N, K, NULL, wg, stream) with a MASKED dX store: the dropout that the consumer of dX --
 * the backward of the BatchNorm + activation + dropout in front of this linear, whose prologue is wg->pro -- would apply
 * first is applied by the producer, and a second producer adds its share:
 *   accumulate == 0:  dX[r, c]  = kept(r, c) ? dx * inv_keep : 0
 *   accumulate != 0:  dX[r, c] += kept(r, c) ? dx * inv_keep : 0       (the product rounded, then ONE fp32 add)
 * kept / inv_keep are those of `mask` (its dropout fields: drop_p, seed / seed_ptr, site, row_offset, over [M, N]).  The
 * kernel takes the keep bits from the hashes its weight-gradient half makes for wg->pro anyway, so `mask` must BE the
 * dropout of wg->pro (equal in those fields; both without dropout: a plain / accumulating store); anything else is refused
 * with MMG_E_ARG before anything is launched.
 * After a write by one pass and an accumulate by another, dX = dropA(dX_A) + dropB(dX_B) in fp32: the consumer then applies
 * the activation's select (mmg_bn_bwd_stats / mmg_linear_bnbwd with the prologue's drop_p = 0) but NO dropout -- bit for
 * bit what mmg_bn_bwd_stats2 / MMG_BNBWD_BN2 form from the two unmasked tensors.  dZ, dW, dbias, dbeta and dgamma are those
 * of mmg_linear_bnbwd.
 * mmg_linear_bnbwd_masked_supported: MMG_BNBWD_BN and MMG_BNBWD_ROWS with a weight gradient, K = N = 128, M > 512. */
int mmg_linear_bnbwd_masked_supported(int mode, int64_t M, int N, int K, int with_wgrad);
int mmg_linear_bnbwd_masked(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                            const mmg_prologue_t* mask, int accumulate, const mmg_bnbwd_wgrad_t* wg, void* stream);
/* Both passes' masked launches of one layer in ONE launch -- the second linear of the encoder under the two dropout passes
 * of a training step.  Bit for bit in every output (dX, both passes' slabs with their jobs, dW, dbias, dbeta, dgamma, and
 * dZ where kept) the two calls
 *   mmg_linear_bnbwd_masked(b, W, dZ_b, dX, M, N, K, wg_b->pro, 0, wg_b, stream)      b->mode == MMG_BNBWD_BN
 *   mmg_linear_bnbwd_masked(a, W, dZ_a, dX, M, N, K, wg_a->pro, 1, wg_a, stream)      a->mode == MMG_BNBWD_ROWS
 * with dX written once and never read back, the shared X [M, N] and W read once, and each 32-row tile walked through pass b
 * and then pass a.  The passes stage one tile of X: wg_b->X == wg_a->X, and the two X prologues agree in everything but
 * the dropout site (scale, shift, relu, drop_p, seed / seed_ptr, row_offset).  Each pass keeps its own slab workspace
 * and job.  Other modes, a missing weight-gradient descriptor and whatever mmg_linear_bnbwd_masked refuses are refused
 * with MMG_E_ARG before anything is launched.
 * mmg_linear_bnbwd_dual_supported: K = N = 128, M > 512. */
int mmg_linear_bnbwd_dual_supported(int64_t M, int N, int K);
int mmg_linear_bnbwd_dual(const mmg_bnbwd_t* b, const mmg_bnbwd_wgrad_t* wg_b, const mmg_bnbwd_t* a,
                          const mmg_bnbwd_wgrad_t* wg_a, const float* W, float* dZ_b, float* dZ_a, float* dX, int64_t M,
                          int N, int K, void* stream);
/* The data gradient AND the weight gradient of a plain linear in ONE launch -- the first layer of a pair head, whose
 * upstream gradient dY [M, K] is the gradient of the head's per-patient table (K = 64) and whose input X [M, N] is the
 * final patient activation (N = 128):
 *   dX [M, N] = dY . W            W stored [K, N], the forward weight in place: mmg_linear_fwd(dY, NULL, W, NULL, dX, M, N, K,
 *                                 MMG_LIN_W_KN, next ? {MMG_EPI_NEXT_BN, next} : NULL)
 *   wg->dW [K, N] (+)= dY^T . pro(X)    mmg_linear_wgrad(dY, wg->X, wg->pro, wg->dW, NULL, M, K, N, wg->accumulate, ...)
 * dY is read and split once and serves both products; dX and dW are bit for bit those of the two calls (same products, same
 * order, same slabs, same slab sum).  wg->dbias must be NULL; wg->pro takes scale / shift and relu, no dropout; the slabs are
 * left in wg->ws and described in *wg->job for mmg_wgrad_reduce_group, job == NULL sums them before returning.
 * next (nullable): the statistics of the BatchNorm backward that consumes dX, from the epilogue.  The layer's input IS that
 * BatchNorm's pre-activation: wg->X must be next->y, and wg->pro and next->pro must agree (scale, shift, relu; no dropout).
 * The partial statistics rows are one per weight-gradient workgroup, so the fp64 summation order differs from
 * mmg_linear_fwd's (the sums are bitwise repeatable from call to call).
 * mmg_linear_dgrad_wgrad_supported: M > 512, N = 128, K = 64, and no dropout in either prologue (drop_p = the larger of
 * the two); anything else is refused with MMG_E_ARG before anything is launched -- the caller then makes the two calls.
 * Workspace: mmg_linear_dgrad_wgrad_ws_bytes(M, N, K) = mmg_linear_wgrad_ws_bytes(M, K, N). */
int mmg_linear_dgrad_wgrad_supported(int64_t M, int N, int K, float drop_p);
size_t mmg_linear_dgrad_wgrad_ws_bytes(int64_t M, int N, int K);
int mmg_linear_dgrad_wgrad(const float* dY, const float* W, float* dX, int64_t M, int N, int K, const mmg_next_bn_t* next,
                           const mmg_bnbwd_wgrad_t* wg, void* stream);

/* Measurement hook (bench.py).  After mmg_probe_arm(n) the next n launches of the big kernels (from any host thread: the
 * backward of a step runs on the autograd engine's thread) carry a HIP start / stop event pair on the kernel itself (hipExtLaunchKernelGGL: the kernel's own begin / end
 * timestamps on its stream -- what rocprofv3 reports -- not a pair of extra queue entries around it).  mmg_probe_read
 * waits for them, disarms the hook and returns how many entries it wrote (<= cap):
 *   ms = kernel duration, tag = MMG_PROBE_* family, (M, N, K) = the launch's shape: rows / output width / inner width for
 *   the dense kernels; patient rows / D / total vocab rows of the fused relations for the aggregates; pairs / 0 / 0 for
 *   the heads;  flags: 1 = accumulate, 4 = prologue, 8 = rowscale, 2048 = the dual linear forward (mmg_linear_fwd_dual: N is
 *   reported as 2 * 128, the two outputs side by side, so that 4 (M K + N K + M N) bytes and 2 M N K FLOP price the launch),
 *   4096 = the layer's weight gradient rides along (mmg_linear_dgrad_wgrad: the row is the data gradient's (M, 128, 64), with
 *   512 where the next-BatchNorm epilogue runs; priced as the data gradient alone, the launch also reads X [M, N] and does
 *   2 M N K FLOP more), 8192 = the masked dX store of mmg_linear_bnbwd_masked (beside the mode's own bits; an accumulating
 *   launch reads dX once more than its row prices), 16384 = the dual backward of mmg_linear_bnbwd_dual (beside 16 | 128 | 1024 |
 *   8192: four [M, 128] inputs -- G and y of pass b, y of pass a, X -- and one output price the launch, the listed rows of
 *   pass a's G and the row list left out), 32768 = a compact second problem rides in the launch (mmg_linear_fwd_rider,
 *   mmg_linear_bnbwd_rider: beside the dense launch's own bits; the rider's rows are left out of the pricing).
 * The hook is the library's only process-wide mutable state (mutex-guarded); the product path never arms it. */
#define MMG_PROBE_LINEAR_FWD 1
#define MMG_PROBE_LINEAR_WGRAD 2
#define MMG_PROBE_LINEAR_WGRAD_REDUCE 3
#define MMG_PROBE_GATHER 4
#define MMG_PROBE_SCATTER 5
#define MMG_PROBE_SCATTER_REDUCE 6
#define MMG_PROBE_PAIR_FWD 7
#define MMG_PROBE_PAIR_BWD 8
#define MMG_PROBE_BN_BWD_STATS 9
#define MMG_PROBE_BN_BWD_APPLY 10
#define MMG_PROBE_ELEMENTWISE 11
#define MMG_PROBE_PAIR_DENSE_FWD 12
#define MMG_PROBE_KNN_IMPUTE 13
int mmg_probe_arm(int n_launches);
#define MMG_PROBE_NAME_LEN 128
/* names (nullable): cap * MMG_PROBE_NAME_LEN bytes; entry i receives the instantiated kernel symbol of launch i, e.g.
 * "k_linear_bnbwd_x6<128, 4, 0>" -- the name rocprofv3 lists the same launch under. */
int mmg_probe_read(float* ms, int* tag, int64_t* M, int* N, int* K, int* flags, char* names, int cap);
/* The launch extents of the entries the LAST mmg_probe_read returned, in its order: grid_xyz (nullable) [cap][3] = gridDim
 * x, y, z; block_x (nullable) [cap] = blockDim.x.  Returns how many it wrote (<= cap).  The persistent kernels walk tiles
 * t0, t0 + G, ...: with this a test reads G -- and so how many tiles a workgroup took -- from the launch that happened. */
int mmg_probe_grids(uint32_t* grid_xyz, uint32_t* block_x, int cap);

/* Row L2 normalisation, F.normalize(p=2, dim=1, eps): out = z / max(||z||, eps); rnorm = 1/max(..) */
int mmg_l2norm_fwd(const float* Z, float* out, float* rnorm, int64_t M, int N, float eps, void* stream);
/* dz = rnorm * (g - out * <out, g>)   (rows whose norm hit eps: dz = g * rnorm)     */
int mmg_l2norm_bwd(const float* G, const float* out, const float* rnorm, float* dZ, int64_t M, int N,
                   float eps, void* stream);

/* Weighted, masked regression loss over the prediction pairs and its gradient in ONE pass
 * (src/train.py:366-386 of the reference: mean(|p - y| * w[lab]) over the supervision subset):
 *   loss = inv_den * sum_k sup[k] * w[k] * (|p_k - y_k|  or  (p_k - y_k)^2)        (fp64 accumulation)
 *   dpred[k] = inv_den * sup[k] * w[k] * (sign(p_k - y_k)  or  2 (p_k - y_k))
 * sup / w may be NULL (= 1).  loss_type 0 = mae, 1 = mse, 2 = huber with delta 1 (compute_regression_loss,
 * src/model.py:579-612: 0.5 d^2 for |d| <= 1, |d| - 0.5 beyond).  `loss` is ONE double on the device.
 * inv_den_ptr (nullable, DEVICE): when non-NULL the normaliser is read from it at run time instead of `inv_den` -- the
 * reference divides by the size of the per-epoch supervision subset (.mean() over pred[mask], train.py:366-386), which
 * changes every epoch while a captured hipGraph keeps its launch arguments. */
size_t mmg_pair_loss_ws_bytes(int64_t n);
int mmg_pair_loss(const float* pred, const float* y, const float* w, const float* sup, int64_t n, double inv_den,
                  const double* inv_den_ptr, int loss_type, float* dpred, double* loss, void* ws, size_t ws_bytes,
                  void* stream);

/* The per-epoch supervision subset (src/train.py:150-176: supervision_mask = torch.rand(n) < mask_fraction, redrawn every
 * epoch from a wall-clock seed) drawn on the device: sup[k] = 1.0f with probability `fraction` (quantised to 1/65536),
 * else 0.0f, from the counter RNG keyed on (seed, a site of its own, ids[k] or k) -- partition-invariant when ids holds
 * global pair ids.  seed_ptr (nullable, DEVICE) overrides `seed` at run time (the dropout seed stream a captured step
 * advances).  count / inv_den (nullable, DEVICE doubles) receive the subset size and 1 / max(size, 1) -- the normaliser
 * mmg_pair_loss reads through inv_den_ptr.  sup == NULL: count only -- a patient-sharded rank draws the mask of ITS pairs
 * (ids = their global ids) and counts the subset of ALL n_global pairs (ids NULL) itself: the draw is a pure function of
 * (seed, id), so every rank gets the global size without a collective.  ids are non-negative and honoured as full
 * 64-bit element indices (any value below 2^63; tested up to 2^40). */
size_t mmg_sup_mask_ws_bytes(int64_t n);
int mmg_sup_mask_draw(const uint64_t* seed_ptr, uint64_t seed, const int64_t* ids, int64_t n, float fraction, float* sup,
                      double* count, double* inv_den, void* ws, size_t ws_bytes, void* stream);

/* keep-mask of the dropout RNG, for injected-mask parity tests: mask[i] in {0,1}     */
int mmg_dropout_mask(uint64_t seed, const uint64_t* seed_ptr, uint32_t site, int64_t first_elem, int64_t n_elems,
                     float p, uint8_t* mask, void* stream);

/* ---------------------------------------------------------------------------------------
 * Degree-gated dual edge head (src/model.py:305-333, EdgeRegressionHead :342-396).
 * The first Linear(2D,64) is split: A = x_P . W1[:, :D]^T (per patient), B = x_lab . W1[:, D:]^T + b1
 * (per lab) -- computed by mmg_linear_fwd -- so that per pair
 *   h1 = drop(relu(A[pi] + B[li])); h2 = drop(relu(W2 h1 + b2)); pred = W3 h2 + b3
 * edge_predictor runs on the final embeddings, tabular_mlp on the initial ones; the head is
 * chosen per pair by deg[pi] < degree_threshold (src/model.py:312-315).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const float* A;          /* [n_patients, 64] */
  const float* B;          /* [n_labs, 64] (bias b1 folded in) */
  const float* W2;         /* [32, 64] */
  const float* b2;         /* [32] */
  const float* W3;         /* [32] */
  const float* b3;         /* [1] */
} mmg_head_t;

typedef struct {
  float* dA;               /* [n_patients, 64]  accumulated (+=) */
  float* dB;               /* [n_labs, 64]      accumulated (+=) */
  float* dW2;              /* [32, 64] += */
  float* db2;              /* [32] += */
  float* dW3;              /* [32] += */
  float* db3;              /* [1] += */
} mmg_head_grad_t;

/* One launch evaluates ONE head on the pairs whose gate matches `want_low`
 * (want_low = 1: deg[pi] < degree_threshold -> tabular_mlp; 0: the GNN edge_predictor);
 * other pairs are left untouched in pred / contribute nothing to the gradients.
 * pair_id (nullable) = original position of each pair, used only to key the dropout RNG so that
 * a permuted (patient-sorted) pair list draws the same masks: the first layer draws elements pair_id * 64 + unit, the
 * second pair_id * 32 + unit, as full 64-bit indices -- any non-negative pair_id with pair_id * 64 < 2^63 (below 2^57;
 * tested up to 2^40).  seed_ptr (nullable, device): overrides
 * `seed` at run time (hipGraph replays).
 * io_perm (nullable, device): the kernels work on a patient-SORTED pair list; io_perm[k] is the position of sorted
 * pair k in the caller's order -- pred is written to pred[io_perm[k]] and dpred read from dpred[io_perm[k]], so no
 * separate permutation pass over the predictions / their gradient is needed.
 * sel / n_sel (both nullable, device): a compacted list of pair positions built by mmg_pair_select -- only
 * sel[0 .. *n_sel) are visited (in list order) and `n_pairs` is then an upper bound of *n_sel that sizes the
 * launch.  Forward: the per-head lists (static per pair set) replace the predicated sweep over all pairs.
 * Backward: pairs whose upstream gradient is exactly 0 (the ~80 % of train pairs outside the supervision
 * subset, src/train.py:366-370) contribute exactly 0 to every gradient and are skipped. */
/* Sizes: n_total = length of pi / li / pair_id / io_perm / pred / dpred; n_patients = rows of A and entries of deg;
 * n_labs = rows of B; n_pairs <= n_total sizes the launch (the list bound, or n_total without a list).  Every indexed
 * access inside the kernels is range-checked against these (buffer descriptors): an index outside its array reads 0 /
 * is not written, it can never become an address.  Limits: n_total < 2^29, n_patients < 2^24, n_labs < 2^24. */
int mmg_pair_head_fwd(const mmg_head_t* head, const int32_t* pi, const int32_t* li,
                      const int32_t* deg, int degree_threshold, int want_low, int64_t n_pairs, int64_t n_total,
                      int64_t n_patients, int n_labs,
                      float drop_p, uint64_t seed, const uint64_t* seed_ptr, const int64_t* pair_id,
                      float* pred, const int32_t* sel, const int32_t* n_sel, const int64_t* io_perm, void* stream);
/* What autograd would save for the backward of the head (model.py:388-396), per pair k of the pair arrays, written by
 * mmg_pair_head_fwd_save for every pair it visits and read by mmg_pair_head_bwd_saved for every pair IT visits (a subset:
 * same head, same gate, pairs with a non-zero upstream gradient):
 *   h1_bits[2 k + w] bit j = [h1[32 w + j] > 0] -- the first layer's activation survived ReLU and dropout, so
 *                            h1 = bit ? (A[pi] + B[li]) / (1 - p) : 0 exactly;
 *   h2[32 k + u]           = the second layer's activation after ReLU and dropout (its sign pattern is the mask).
 * The backward then needs no RNG, no second-layer product and no epilogue arithmetic per pair (136 B per pair instead);
 * NULL `saved` = the plain entry points: the backward recomputes -- in the forward's own order, so both variants return
 * the same bits.  Up to 64 labs on the backward side (beyond: recomputed). */
typedef struct {
  uint32_t* h1_bits;      /* [n_entries, 2] */
  float* h2;              /* [n_entries, 32] */
  int by_position;        /* != 0: entry = position in the pair list `sel` instead of the pair index k -- dense, streamed
                           * writes and reads; the backward must then run over the SAME list as the forward */
  int64_t n_entries;      /* rows of both buffers: >= n_total (indexed by pair), >= n_pairs -- the launch bound of the list
                           * -- when by_position; checked by both entry points (MMG_ERR_ARG) */
} mmg_pair_saved_t;
int mmg_pair_head_fwd_save(const mmg_head_t* head, const int32_t* pi, const int32_t* li,
                           const int32_t* deg, int degree_threshold, int want_low, int64_t n_pairs, int64_t n_total,
                           int64_t n_patients, int n_labs,
                           float drop_p, uint64_t seed, const uint64_t* seed_ptr, const int64_t* pair_id,
                           float* pred, const int32_t* sel, const int32_t* n_sel, const int64_t* io_perm,
                           const mmg_pair_saved_t* saved, void* stream);
/* Dense imputation: ONE head over every lab of a list of patient rows, no pair list --
 *   out[out_rows[r] * ld_out + l] = head(A[rows[r]], B[l])   for r < n_rows, l < n_labs  (inference: no dropout).
 * Bitwise what mmg_pair_head_fwd returns for the pair (rows[r], l) with drop_p = 0 on the same head: same arithmetic in
 * the same order (the caller applies the degree gate by choosing the head per row).  rows index A ([n_patients, 64]);
 * out is [n_out, ld_out] fp32; other rows and the columns n_labs .. ld_out-1 are left untouched.  Every indexed access
 * is range-checked: a rows[r] outside [0, n_patients) or an out_rows[r] outside [0, n_out) skips that row (rows /
 * out_rows / A / B through buffer descriptors; out in 64-bit offsets, so it may exceed 4 GiB).  Requests of 2^31 cells
 * or more are split into several launches on `stream`.  Limits: n_patients < 2^24, n_labs < 2^24, ld_out >= n_labs.
 * Argument errors (MMG_E_ARG) are found on the host before anything is enqueued. */
int mmg_pair_head_dense_fwd(const mmg_head_t* head, const int32_t* rows, const int32_t* out_rows, int64_t n_rows,
                            int64_t n_patients, int n_labs, float* out, int64_t n_out, int64_t ld_out, void* stream);
/* Backward: the weight-side gradients (dW2, db2, dW3, db3, dB) leave every workgroup as ONE partial slab in `ws` and are
 * summed in fixed order (bitwise reproducible); dA rows are flushed per patient run (pairs sorted by patient: a row
 * receives at most two partial sums unless one patient holds more than 32 listed pairs). */
size_t mmg_pair_head_bwd_ws_bytes(int64_t n_pairs, int n_labs);
int mmg_pair_head_bwd(const mmg_head_t* head, const mmg_head_grad_t* grad,
                      const int32_t* pi, const int32_t* li, const int32_t* deg, int degree_threshold,
                      int want_low, int64_t n_pairs, int64_t n_total, int64_t n_patients, int n_labs, float drop_p,
                      uint64_t seed,
                      const uint64_t* seed_ptr, const int64_t* pair_id, const float* dpred,
                      const int32_t* sel, const int32_t* n_sel, const int64_t* io_perm,
                      void* ws, size_t ws_bytes, void* stream);
int mmg_pair_head_bwd_saved(const mmg_head_t* head, const mmg_head_grad_t* grad,
                            const int32_t* pi, const int32_t* li, const int32_t* deg, int degree_threshold,
                            int want_low, int64_t n_pairs, int64_t n_total, int64_t n_patients, int n_labs, float drop_p,
                            uint64_t seed,
                            const uint64_t* seed_ptr, const int64_t* pair_id, const float* dpred,
                            const int32_t* sel, const int32_t* n_sel, const int64_t* io_perm,
                            const mmg_pair_saved_t* saved, void* ws, size_t ws_bytes, void* stream);

/* Stable two-way compaction of pair positions by head: position k goes to sel_low if deg[pi[k]] < threshold,
 * else to sel_high -- and only if dpred is NULL or dpred[k] != 0.  Order inside a list = pair order (pairs sorted
 * by patient stay sorted).  counts[0], counts[1] (device) = list lengths.  sel_low / sel_high: capacity n each.
 * dpred is read through io_perm (nullable); dpred_sorted (nullable, [n]) receives dpred in pair order -- the ONE
 * random pass over the gradient -- for mmg_pair_head_bwd to read sequentially (with io_perm = NULL). */
size_t mmg_pair_select_ws_bytes(int64_t n_pairs);
int mmg_pair_select(const int32_t* pi, const int32_t* deg, int degree_threshold, const float* dpred,
                    const int64_t* io_perm, float* dpred_sorted, int64_t n_pairs, int32_t* sel_low, int32_t* sel_high,
                    int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* The supervision subset of a step AND the two pair lists derived from it, in two launches: what mmg_sup_mask_draw
 * followed by mmg_pair_select(pi, deg, threshold, sup, io_perm) gives, bit for bit, without reading a mask back.
 *   s = 0 .. n_pairs-1 (patient-sorted position):  c = io_perm ? io_perm[s] : s  (the caller's index of that pair),
 *   e = ids ? ids[c] : c  (its id),  supervised(s) = mmg_sup_mask_draw's draw for id e with the same seed and fraction,
 *   low(s) = deg[pi[s]] < degree_threshold
 * sel_low / sel_high (capacity n_pairs each) receive the supervised positions of each head in increasing order, counts[2]
 * (device) their lengths; count / inv_den (nullable, DEVICE doubles) the subset size (double)(counts[0] + counts[1]) and
 * 1 / max(size, 1); sup (nullable, [n_pairs] float, CALLER order) the mask mmg_pair_loss reads: sup[c] = 1.0f or 0.0f.
 * seed_ptr (nullable, DEVICE) overrides `seed` at run time; ids (nullable) as in mmg_sup_mask_draw.  pi is in sorted
 * order, io_perm a permutation of 0 .. n_pairs-1 (or NULL: the pairs are sorted as the caller has them).
 * Launch 1 hashes every position and leaves per-workgroup totals (and writes sup, sequentially); launch 2 scans the totals
 * and emits the lists.  No workgroup waits for another one: the stream orders the two launches.  max_groups: 0, or the
 * number of workgroups to use at most (1 .. 1024; a test walks several chunks per workgroup with a small one).
 * n_pairs == 0: counts = {0, 0}, count = 0, inv_den = 1. */
size_t mmg_sup_draw_select_ws_bytes(int64_t n_pairs);
int mmg_sup_draw_select(const uint64_t* seed_ptr, uint64_t seed, float fraction, const int64_t* ids,
                        const int64_t* io_perm, const int32_t* pi, const int32_t* deg, int degree_threshold,
                        int64_t n_pairs, int max_groups, float* sup, int32_t* sel_low, int32_t* sel_high, int32_t* counts,
                        double* count, double* inv_den, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Grouped launches for the vocab side (tables of 50 .. 200 rows: every lin_l / lin_r of a SAGEConv into a vocab type, the
 * transformed tables the patient-side gather reads, their weight / data gradients -- src/model.py:125-131,256 -- is a few
 * microseconds of work behind a launch).  One launch runs up to MMG_SMALL_MAX independent problems of one (N, K).
 *   mmg_small_fwd_group  : Y[M,N] (+)= X[M,K] . W^T (+ X2[M,K] . W2^T) + bias ;  flags as mmg_linear_fwd
 *                          (MMG_LIN_ACCUMULATE, MMG_LIN_W_KN: both W and W2 stored [K,N]);  exact fp32 products
 *   mmg_small_wgrad_group: dW[N,K] (+)= dY[M,N]^T . X[M,K] ;  dbias[N] (nullable) (+)= column sums of dY
 * M <= 4096 per problem (M = 0: skipped by the forward, zero / untouched gradient by the weight gradient).
 * ------------------------------------------------------------------------------------- */
#define MMG_SMALL_MAX 8
typedef struct {
  const float* X; const float* W;      /* [M,K], [N,K] (or [K,N]) */
  const float* X2; const float* W2;    /* optional second term, both NULL or both set */
  const float* bias;                   /* [N] or NULL */
  float* Y;                            /* [M,N] */
  int64_t M;
  int flags;
} mmg_small_fwd_t;
typedef struct {
  const float* dY; const float* X;     /* [M,N], [M,K] */
  float* dW; float* dbias;             /* [N,K], [N] or NULL */
  int64_t M;
  int accumulate;
} mmg_small_wgrad_t;
int mmg_small_fwd_group(const mmg_small_fwd_t* probs, int n_probs, int N, int K, void* stream);
int mmg_small_wgrad_group(const mmg_small_wgrad_t* probs, int n_probs, int N, int K, void* stream);

/* The per-type epilogue of a HeteroConv layer (src/model.py:258-269: BatchNorm1d -> activation -> Dropout) for every
 * SMALL node type in one launch, and its backward in another.  Per problem (M <= 4096 rows):
 *   forward : training: batch statistics (fp64 sums) -> scale / shift / mean / rstd written to stats_out[4,N] (the layout
 *             mmg_bn_finalize produces), running statistics advanced once (unbiased variance, `momentum`);  eval: folded
 *             from the running statistics;  gamma == NULL: no BatchNorm.  out = dropout(act(Y * scale + shift)).
 *   backward: g' = G * act'(.) * keep / (1 - p);  training: dY = scale (g' - mean g' - xhat mean(g' xhat)), dbeta = sum g',
 *             dgamma = sum g' xhat;  eval: dY = scale g';  scale == NULL: dY = g'.
 * Dropout masks are the ones mmg_affine_act_drop draws for the same (seed, site, row_offset). */
typedef struct {
  const float* Y; float* out;           /* [M,N] */
  const float* gamma; const float* beta; float* running_mean; float* running_var;   /* [N]; gamma NULL = no BatchNorm */
  float* stats_out;                     /* [4,N]: scale | shift | mean | rstd */
  int64_t M;
  int training;
  int act;                              /* MMG_ACT_* */
  float drop_p;
  uint64_t seed; uint32_t site; int64_t row_offset; const uint64_t* seed_ptr;
} mmg_small_bn_t;
typedef struct {
  const float* G; const float* Y; float* dY;                                  /* [M,N] */
  const float* scale; const float* shift; const float* mean; const float* rstd;   /* [N]; scale NULL = no BatchNorm */
  float* dbeta; float* dgamma;                                                 /* [N], nullable */
  int64_t M;
  int training;
  int act;
  float drop_p;
  uint64_t seed; uint32_t site; int64_t row_offset; const uint64_t* seed_ptr;
} mmg_small_bn_bwd_t;
int mmg_small_bn_act_group(const mmg_small_bn_t* probs, int n_probs, int N, float momentum, float eps, void* stream);
int mmg_small_bn_bwd_group(const mmg_small_bn_bwd_t* probs, int n_probs, int N, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimizer step (src/train.py:219,390: torch.optim.Adam(model.parameters()).step()) and small vector sums.
 * mmg_adam_step updates EVERY parameter in one launch: p / m / v are flat fp32 buckets holding the tensors back to back
 * at offsets[0 .. n_tensors] (ascending, offsets[n_tensors] = end); grads[i] (HOST array of device pointers; NULL = the
 * tensor received no gradient and is left untouched, as torch skips a .grad of None) is read where the backward kernels
 * wrote it.  Arithmetic of torch.optim.Adam (amsgrad / maximize off, L2 weight decay added to the gradient).  `step`
 * (device float, the number of steps taken so far) is advanced by a one-thread launch behind the update -- hipGraph
 * replays keep counting.  `ticket` (device uint32) is no longer used (the last-workgroup scheme it served cost a
 * device-scope fence per workgroup) and stays in the signature for the ABI.
 * mmg_vec_sums: dst_j = src_j0 (+ src_j1 + src_j2 + src_j3), fixed order, <= MMG_SUM_MAX_JOBS jobs per launch (the
 * three lin_r weights / lin_l biases that share x_patient in a HeteroConv layer, src/model.py:125-131; the gradient
 * contributions of a parameter that is used twice).  A job is a [len / cols, cols] matrix with its own row stride on
 * every side (cols = 0: a flat vector), so the same launch also takes the two halves of an edge head's first-layer
 * weight W1[:, :D] | W1[:, D:] apart (src/model.py:375-382: the head's Linear(2D, H)) and puts their gradients together.
 * mmg_counters_add: *counters[i] += incs[i] for <= MMG_SUM_MAX_JOBS * 4 int64 counters (BatchNorm1d.num_batches_tracked
 * of every layer in one launch).  mmg_seed_advance: state[1] += 1 step of a SplitMix64 stream, state[0] = its output
 * (< 2^62) -- the dropout seed the kernels read through mmg_prologue_t.seed_ptr, advanced inside a captured step.
 * mmg_fill_zero: zero-fill by a kernel on `stream` (bytes of any count / alignment).  Not hipMemsetAsync: recorded into a
 * hipGraph its node replays a pattern other than the recorded zero on this ROCm (profiles/probes/hipgraph_memset_node.py).
 * ------------------------------------------------------------------------------------- */
#define MMG_ADAM_MAX_TENSORS 96
#define MMG_SUM_MAX_JOBS 8
int mmg_adam_step(float* p, float* m, float* v, const float* const* grads, const int32_t* offsets, int n_tensors,
                  float lr, float beta1, float beta2, float eps, float weight_decay, float* step, uint32_t* ticket,
                  void* stream);
/* The same step with its hyper-parameters read from DEVICE memory at run time: hyper[5] = (lr, beta1, beta2, eps,
 * weight_decay).  A captured hipGraph keeps its launch arguments, so a learning-rate scheduler (src/train.py:271-291:
 * ReduceLROnPlateau / StepLR acting on optimizer.param_groups) would be silently ignored by mmg_adam_step under replay;
 * the caller refreshes `hyper` between replays instead. */
int mmg_adam_step_dev(float* p, float* m, float* v, const float* const* grads, const int32_t* offsets, int n_tensors,
                      const float* hyper, float* step, uint32_t* ticket, void* stream);
/* mmg_adam_step_dev's update launches WITHOUT the one-thread launch that advances `step`: the caller advances it behind
 * them, with mmg_step_advance. */
int mmg_adam_update_dev(float* p, float* m, float* v, const float* const* grads, const int32_t* offsets, int n_tensors,
                        const float* hyper, float* step, void* stream);
typedef struct {
  float* dst;
  const float* src[4];
  int n_src;               /* 1..4 */
  int len;                 /* elements */
  int cols;                /* 0: flat;  > 0: rows of `cols` elements (len % cols == 0) with the strides below */
  int ld_dst;              /* row stride of dst (elements) */
  int ld_src[4];           /* row stride of every source */
} mmg_sum_job_t;
int mmg_vec_sums(const mmg_sum_job_t* jobs, int n_jobs, void* stream);
/* Everything that finishes the gradients of a step, in ONE launch: the slab sums of mmg_wgrad_reduce_group, the sums of
 * further contributions of mmg_vec_sums, and the placement of a sum inside a wider matrix -- described with the job
 * types of those two calls.  One job = one destination; per element, in this order:
 *   (a) `series`, in list order: an entry is summed as mmg_wgrad_reduce_group sums it (16 slab groups, group g adds its
 *       slabs g, g + 16, ... in turn, then part[0] + ... + part[15]) and stored, or added to its dW with `accumulate`.  A
 *       later entry with the same dW (and n4, nk4, dbias; accumulate != 0; up to MMG_GRAD_FINISH_SERIES entries per dW) is
 *       a further series of that job: its finished sum is added to the value -- what one launch per entry gives.
 *   (b) `sums`, mmg_vec_sums jobs.  A sum whose src[0] is EXACTLY the dW of a series job (len = 4 * nk4, n_src <= 4, at
 *       most one such sum per dW) belongs to that job: value = (a) + src[1] + src[2] + src[3], in mmg_vec_sums' order, and
 *   (c) the store goes to the sum's dst with its cols / ld_dst -- dW itself when dst == dW, else a column slice of a
 *       wider matrix, and dW is then NOT written (nobody may read it); the dbias tail goes to dbias either way.  With
 *       slabs, addresses, cols and strides are multiples of four elements.  Every other sum is a job of its own, as in
 *       mmg_vec_sums (any length, any alignment).
 * The jobs of a launch run concurrently: a job that reads what another job writes (or a dW left unwritten), and two jobs
 * whose destinations overlap, are refused with MMG_E_ARG before anything is launched (such a job belongs in a later
 * launch); column slices of one matrix with the same row stride are told apart.  More than MMG_GRAD_FINISH_MAX jobs (the
 * table travels by value in the kernarg segment) take several launches, and the rule holds across them.  NULL
 * destinations, sources or slabs are refused. */
#define MMG_GRAD_FINISH_MAX 24
#define MMG_GRAD_FINISH_SERIES 4
int mmg_grad_finish_group(const mmg_wgrad_reduce_t* series, int n_series, const mmg_sum_job_t* sums, int n_sums,
                          void* stream);
#define MMG_COUNTERS_MAX 32
int mmg_counters_add(int64_t* const* counters, const int64_t* incs, int n, void* stream);
int mmg_seed_advance(uint64_t* state /* [2]: seed | stream position */, void* stream);
/* The one-thread updates that end a captured training step, in ONE launch: *adam_step += 1 (what mmg_adam_step* launch
 * behind their update), mmg_seed_advance(seed_state) and mmg_counters_add(counters, incs, n_counters).  adam_step NULL,
 * seed_state NULL, n_counters 0: that part is left out. */
int mmg_step_advance(float* adam_step, uint64_t* seed_state, int64_t* const* counters, const int64_t* incs, int n_counters,
                     void* stream);
int mmg_fill_zero(void* ptr, size_t bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Evaluation reducers on the device (src/evaluate.py:36-82 metrics, :417-440 per-lab +-3 sigma winsorisation, :89-141
 * per-lab rows, :237-342 stratifications).  Every figure evaluate_model reports is a segment sum over the prediction
 * pairs (segment = lab index, patient-degree bucket, lab-frequency bucket; seg[k] outside [0, n_seg) = not counted), so
 * the predictions stay on the device and [n_seg, 8] doubles come back.
 *   mmg_seg_moments: moments[s] = (n, sum r, sum r^2), r = pred - target.
 *   mmg_seg_metrics: residuals clipped to mean +- n_sigma * std of their segment (population std, segments with > 1
 *     sample; n_sigma <= 0 or moments NULL: none), adjusted prediction = target + clipped residual (written to
 *     pred_out when non-NULL); sums[s] = (n, sum |e|, sum e^2, sum t, sum t^2, sum |e/t| over t != 0, count(t != 0),
 *     count(clipped)) with e = t - adjusted prediction.  fp64 accumulation.  n_seg <= 2048.
 * ------------------------------------------------------------------------------------- */
size_t mmg_seg_reduce_ws_bytes(int64_t n, int n_seg);
int mmg_seg_moments(const float* pred, const float* target, const int64_t* seg, int64_t n, int n_seg,
                    double* moments, void* ws, size_t ws_bytes, void* stream);
int mmg_seg_metrics(const float* pred, const float* target, const int64_t* seg, int64_t n, int n_seg,
                    const double* moments, float n_sigma, float* pred_out, double* sums, void* ws, size_t ws_bytes,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Nearest-neighbour lab imputation: sklearn.impute.KNNImputer(n_neighbors, weights).fit_transform(X) on the device
 * (the reference config's evaluation.baselines "nearest_neighbor"; mmgnn/knn.py).  X is a dense [n_rows, ld_x] fp32
 * patient x lab matrix, NaN = missing; every row is both a donor and a receiver.  For i < n_out and l < n_cols:
 *   out[i * ld_out + l] = X[r, l] when it is observed (r = rows[i]); otherwise, over the donors D_l = {d : X[d, l]
 *   observed} (never r itself) at nan-Euclidean distance dist(r, d) = sqrt(n_cols * S / c) -- c = labs both observe,
 *   S = sum of (X[r, j] - X[d, j])^2 over them, NaN when c = 0 -- the weighted mean of X[d, l] over the min(k, |D_l|)
 *   donors of smallest (dist, d), NaN last: weights 0 (uniform) 1 per finite distance, 1 (distance) 1 / dist, or
 *   [dist == 0] when a chosen distance is 0; NaN distances weigh 0.  Every donor at a NaN distance: the fp64 mean of
 *   the observed X[:, l] rounded to fp32; D_l empty: NaN (sklearn drops such a column).
 * Distances are direct masked fp32 sums in lab order (no |x|^2 + |y|^2 - 2xy expansion) from the original X, and the
 * selection is a total order on (S / c, d), so every output cell is bitwise reproducible and does not depend on which
 * other rows are requested.  A rows[i] outside [0, n_rows) skips output row i; columns n_cols .. ld_out-1 and skipped
 * rows are left untouched.  Limits: 1 <= n_cols <= 512, 1 <= n_neighbors <= 32, 0 <= n_rows < 2^31, 0 <= n_out < 2^31,
 * ld_x >= n_cols, ld_out >= n_cols (MMG_E_ARG); ws: mmg_knn_impute_ws_bytes (the column means; MMG_E_WS).  Every
 * argument is checked on the host before anything is enqueued.  Cost O(n_out * n_rows * observed labs).
 * ------------------------------------------------------------------------------------- */
size_t mmg_knn_impute_ws_bytes(int64_t n_rows, int n_cols, int64_t n_out, int n_neighbors);
int mmg_knn_impute(const float* X, int64_t n_rows, int n_cols, int64_t ld_x, const int32_t* rows, int64_t n_out,
                   int n_neighbors, int weights /* 0 uniform, 1 distance */, float* out, int64_t ld_out, void* ws,
                   size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Leakage-audit reducers (src/audit_leakage.py; mmgnn/audit.py).  Every argument is checked on the host before anything
 * is enqueued (MMG_E_ARG; a short workspace MMG_E_WS); no call synchronises with the host, so each one can be captured.
 *
 * mmg_order_stats: out[r] = the value of 0-based rank ranks[r] (a HOST array, 0 <= rank < n) of the n keys in ascending
 *   order, NaN last (numpy's sort order; -0 and +0 are ordered by sign, which np.partition does not promise).  The keys
 *   are a[i] (b NULL) or |a[i] - b[i]| formed in fp32 (numpy's abs(y_pred - y_true)).  nan_count (device, nullable):
 *   the number of NaN keys.  Exact: an 11 / 11 / 10-bit radix select with integer histograms, three histogram launches
 *   and three one-workgroup selection steps.  1 <= n < 2^31, 1 <= n_ranks <= MMG_OS_MAX_RANKS.
 * ------------------------------------------------------------------------------------- */
#define MMG_OS_MAX_RANKS 8
size_t mmg_order_stats_ws_bytes(int64_t n);
int mmg_order_stats(const float* a, const float* b, int64_t n, const int64_t* ranks, int n_ranks, float* out,
                    int64_t* nan_count, void* ws, size_t ws_bytes, void* stream);

/* mmg_robust_sums: one pass over (pred, target), r = pred - target in fp32, for compute_robust_metrics.  The winsorising
 * bounds are numpy's "linear" percentiles of |r|, formed on the device from the order statistics xs[0 .. n_xs) of
 * mmg_order_stats (mode |a - b|) and its nan_count (any NaN: the percentile is NaN):
 *   x_i = xs[p.lo], x_j = xs[p.hi], d = x_j - x_i, value = p.g >= 0.5 ? x_j - d * (1 - p.g) : x_i + d * p.g
 * every operation rounded in fp32 on its own (no fused multiply-add); the host derives (lo, hi, g) from n and the
 * percentile as numpy does.  out (device, fp64 [MMG_RS_FIELDS]):
 *   n, sum |r|, sum r^2, sum t, sum t^2, sum |r| / (|t| + |p| + 1e-8f) (the fp32 SMAPE term), sum |t|,
 *   sum clip(|r|, lower, upper), sum clip(r, -upper, upper)^2, count(|r| < lower or |r| > upper), count(NaN |r|),
 *   max |r| (NaN if any is NaN), lower, upper, p95.
 * fp64 sums over the fp32 terms in a fixed order (per-workgroup rows added in row order): bitwise reproducible. */
typedef struct {
  int32_t lo, hi; /* indices into xs of the two order statistics */
  float g;        /* interpolation weight (fp32, numpy's gamma) */
} mmg_percentile_t;
#define MMG_RS_FIELDS 15
#define MMG_RS_LOWER 12
#define MMG_RS_UPPER 13
#define MMG_RS_P95 14
size_t mmg_robust_sums_ws_bytes(int64_t n);
int mmg_robust_sums(const float* pred, const float* target, int64_t n, const float* xs, int n_xs,
                    const int64_t* nan_count, mmg_percentile_t lower, mmg_percentile_t upper, mmg_percentile_t p95,
                    double* out, void* ws, size_t ws_bytes, void* stream);

/* mmg_split_membership: patient[e] (int64) of every has_lab edge and the three bool (one byte) split masks.  Every
 * patient in [0, n_patients) gets the word OR of 1 << split over its edges; counts (device, int64 [MMG_SM_FIELDS]):
 *   counts[m], m = 1..7: patients whose word is m (counts[0] = 0: patients without a masked edge are not counted),
 *   counts[8]: edges in more than one split, counts[9]: edges in train and in val or test.
 * Patient ids outside [0, n_patients) are not counted.  Integer counts: exact. */
#define MMG_SM_FIELDS 10
size_t mmg_split_membership_ws_bytes(int64_t n_patients);
int mmg_split_membership(const int64_t* patient, const uint8_t* train_mask, const uint8_t* val_mask,
                         const uint8_t* test_mask, int64_t n_edges, int64_t n_patients, int64_t* counts, void* ws,
                         size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Lab-event preprocessing (src/preprocess.py:28-164, src/utils.py:309-481; mmgnn/preprocess.py).  Events are device
 * arrays over n rows: lab and patient as int64 codes (code order = key order; a code outside [0, n_labs) /
 * [0, n_patients) means "not selected" / "not in the cohort": the row is ignored and never used as an address), value
 * fp64, time int64 with INT64_MAX for a missing time.  All value arithmetic is fp64, every operation rounded on its own
 * (no fused multiply-add), no floating-point atomics: results are bitwise reproducible.  0 <= n < 2^31,
 * 1 <= n_patients < 2^31, 1 <= n_labs <= MMG_PREP_MAX_LABS; n = 0 is valid.  Every argument is checked on the host
 * before anything is enqueued (MMG_E_ARG; a short workspace MMG_E_WS).  ONLY mmg_lab_aggregate synchronises with the
 * host (its pair count sizes the caller's outputs); the other calls can be captured.
 *
 * Per-lab table: stats [n_labs][MMG_LS_FIELDS] fp64, fields MMG_LS_*.  N counts the non-NaN values, ROWS all rows; a lab
 * without a valid value has N = 0 and NaN elsewhere ("stats[lab] = None" of the reference: its values pass through).
 * ------------------------------------------------------------------------------------- */
#define MMG_PREP_MAX_LABS 2048
#define MMG_LS_FIELDS 9
#define MMG_LS_N 0
#define MMG_LS_MEAN 1
#define MMG_LS_STD 2 /* ddof = 1; NaN for N <= 1 */
#define MMG_LS_MIN 3
#define MMG_LS_MAX 4
#define MMG_LS_Q25 5
#define MMG_LS_MEDIAN 6
#define MMG_LS_Q75 7
#define MMG_LS_ROWS 8
#define MMG_PS_TIME 0  /* secondary key: int64 time, ascending, INT64_MAX (missing) last */
#define MMG_PS_VALUE 1 /* secondary key: fp64 value, ascending, every NaN last */
#define MMG_AGG_LAST 0
#define MMG_AGG_MEAN 1
#define MMG_AGG_MEDIAN 2
#define MMG_AGG_MIN 3
#define MMG_AGG_MAX 4
#define MMG_OUT_NONE 0
#define MMG_OUT_STD 1 /* remove v < mean - t * std or v > mean + t * std */
#define MMG_OUT_IQR 2 /* remove v < q25 - t * iqr or v > q75 + t * iqr */
#define MMG_NORM_ZSCORE 0
#define MMG_NORM_MINMAX 1
#define MMG_NORM_ROBUST 2
#define MMG_LT_OUTLIER 0
#define MMG_LT_NORMALIZE 1
#define MMG_LT_INVERSE 2

/* mmg_prep_sort: perm [n] = the row ids in ascending (group, secondary key) order, group = lab * n_patients + patient
 * (patient NULL: group = lab), ties in input order (a stable LSD radix sort; secondary NULL: the group alone).  Ignored
 * rows come last under the group n_labs * n_patients.  group_sorted [n] = the group at every sorted position;
 * value_sorted [n] (nullable, with value_src) = value_src[perm[i]].  The digit passes of the secondary key in which
 * every key agrees move the data unchanged (decided on the device from the OR / AND of the keys). */
size_t mmg_prep_sort_ws_bytes(int64_t n);
int mmg_prep_sort(const int64_t* lab, const int64_t* patient, const void* secondary, int kind, int64_t n,
                  int64_t n_patients, int n_labs, const double* value_src, int32_t* perm, int64_t* group_sorted,
                  double* value_sorted, void* ws, size_t ws_bytes, void* stream);

/* mmg_lab_stats: N, MEAN, STD, MIN, MAX, ROWS of every lab over a lab-sorted array (group_sorted / n_patients = the
 * lab; n_patients = 1 for an array of lab codes), NaN-skipping, pandas' two-pass variance; the quantile fields are set to
 * NaN.  mmg_lab_quantiles: Q25, MEDIAN, Q75 from a (lab, value)-sorted array (mmg_prep_sort with MMG_PS_VALUE): numpy's
 * "linear" interpolation x_i + (x_j - x_i) * g, or x_j - (x_j - x_i) * (1 - g) for g >= 0.5; the median of an even
 * count is (a + b) / 2. */
size_t mmg_lab_stats_ws_bytes(int n_labs);
int mmg_lab_stats(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients, int n_labs,
                  double* stats, void* ws, size_t ws_bytes, void* stream);
size_t mmg_lab_quantiles_ws_bytes(int n_labs);
int mmg_lab_quantiles(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients, int n_labs,
                      double* stats, void* ws, size_t ws_bytes, void* stream);

/* mmg_lab_aggregate: one value per (patient, lab) segment of the sorted events, in (lab, patient) order.  With an
 * outlier method the values outside the lab's bounds (from stats) and the NaN values leave first, and a segment with no
 * row left gives no pair; without one every row stays and a NaN can be the result.  MMG_AGG_LAST takes the last
 * remaining row of the segment (sort with MMG_PS_TIME: the greatest time, among equal times the last in input order, a
 * missing time wins); MEDIAN needs the MMG_PS_VALUE order; MEAN / MIN / MAX / MEDIAN skip NaN (none left: NaN).
 * Outputs hold up to n entries; *n_pairs (HOST) receives the count -- this call waits for the stream. */
size_t mmg_lab_aggregate_ws_bytes(int64_t n);
int mmg_lab_aggregate(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients, int n_labs,
                      int method, int outlier_method, double threshold, const double* stats, int64_t* out_patient,
                      int64_t* out_lab, double* out_value, int64_t* n_pairs, void* ws, size_t ws_bytes, void* stream);

/* mmg_lab_transform: out[i] from value[i] and the table row of lab[i] (lab NULL: row 0 for every element).
 *   MMG_LT_OUTLIER (method MMG_OUT_STD / MMG_OUT_IQR): NaN where the value lies outside the bounds, else the value;
 *   MMG_LT_NORMALIZE (method MMG_NORM_*): zscore (std 0 or NaN: v - mean), minmax (range 0 or NaN: v * 0), robust (iqr 0
 *   or NaN: v - median); MMG_LT_INVERSE: v * spread + location, with no special case for a zero spread.
 * mmg_lab_inverse_matrix: the inverse of a dense fp32 [n_rows, n_labs] matrix (column c = lab c), formed in fp64 and
 * rounded once. */
int mmg_lab_transform(int mode, int method, double threshold, const int64_t* lab, const double* value, int64_t n,
                      int n_labs, const double* stats, double* out, void* stream);
int mmg_lab_inverse_matrix(int method, const float* pred, int64_t n_rows, int n_labs, int64_t ld, const double* stats,
                           float* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Prediction-analysis reducers (src/advanced_visualizations.py: per-lab calibration, error against patient lab-degree,
 * parity by lab-frequency decile; mmgnn/analysis.py).  A pair is (pred[i], target[i], patient[i], lab[i]); the indices
 * are int64 (index_bytes 8) or int32 (4) and are narrowed in the kernel's load.  An index outside [0, n_labs) /
 * [0, n_patients) takes the pair out of the lab sums / the bin sums and is never used as an address.  The degree bins are
 * half open: bin j takes deg[patient] in [bin_edges[j], bin_edges[j + 1]) (a HOST array of n_bins + 1 ascending values,
 * +-inf allowed); a pair outside every bin is counted in none.  n_labs = 0 (lab NULL) leaves the lab part out, n_bins = 0
 * (patient, deg NULL) the bin part.
 *
 * mmg_pair_analysis: ONE read of the pairs.  lab_sums (device, fp64 [n_labs][MMG_AN_LAB_FIELDS]):
 *   n, sum t, sum p, sum t^2, sum t p, sum |p - t|, sum (p - t)^2, min t, max t   (min / max of a lab without a pair:
 *   +inf / -inf); bin_sums (device, fp64 [n_bins][MMG_AN_BIN_FIELDS]): n, sum |p - t|.  p - t, |p - t| and (p - t)^2
 *   are formed in fp32, as numpy forms them on fp32 arrays; t^2 and t p are exact in fp64.
 * mmg_pair_calibrated_abs: the second read.  lab_abs (fp64 [n_labs]) = sum |(a[lab] t + b[lab]) - t| with a, b fp32
 *   (device, [n_labs]) and every operation rounded in fp32 on its own (numpy's a * targets + b on fp32 operands);
 *   bin_sq (fp64 [n_bins]) = sum (|p - t| - bin_mean[bin])^2 in fp64 (bin_mean: device, fp64 [n_bins]).  With
 *   n_bins = 0 pred and patient are not read; with n_labs = 0 lab is not read.
 * fp64 accumulation without floating-point atomics in an order fixed by n, the table sizes and the order of the pairs:
 * bitwise reproducible from run to run (csrc/analysis.hip).  Limits: 0 <= n < 2^31, n_labs <= 2048,
 * n_bins <= MMG_AN_MAX_BINS and 64 n_labs + 768 n_bins <= 163840 (the LDS of one wave; otherwise MMG_E_ARG -- the
 * caller falls back to host arithmetic).  Every argument is checked on the host before anything is enqueued
 * (MMG_E_ARG; a short workspace MMG_E_WS); no call synchronises with the host, allocates or uses a memset node, so
 * each one can be captured.
 * ------------------------------------------------------------------------------------- */
#define MMG_AN_MAX_BINS 64
#define MMG_AN_LAB_FIELDS 9
#define MMG_AN_BIN_FIELDS 2
size_t mmg_pair_analysis_ws_bytes(int64_t n, int n_labs, int n_bins);
int mmg_pair_analysis(const float* pred, const float* target, const void* patient, const void* lab, int index_bytes,
                      int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                      double* lab_sums, double* bin_sums, void* ws, size_t ws_bytes, void* stream);
size_t mmg_pair_calibrated_abs_ws_bytes(int64_t n, int n_labs, int n_bins);
int mmg_pair_calibrated_abs(const float* pred, const float* target, const void* patient, const void* lab, int index_bytes,
                            int64_t n, int n_labs, const float* a, const float* b, const int32_t* deg,
                            int64_t n_patients, const double* bin_edges, int n_bins, const double* bin_mean,
                            double* lab_abs, double* bin_sq, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Feature-space selection (src/io_mimic.py filter_labs_for_cohort, src/preprocess.py process_diagnoses /
 * process_medications; mmgnn/preprocess.py, csrc/select.hip): which codes become nodes and which event rows stay.
 * Events are device arrays over n rows: code and patient as int64 (code order = key order; a code outside
 * [0, n_codes) means the row is ignored, a patient outside [0, n_patients) means "not in the cohort" and the row is
 * ignored; neither is ever used as an address), valid uint8 (nullable; 0 = the row is ignored -- for labs
 * VALUENUM.notna()).  The remaining rows are the COUNTED rows.
 *   n_patients_per_code [n_codes] int64: distinct patients among the counted rows (NUM_PATIENTS; value_counts of the
 *     de-duplicated pairs);  n_rows_per_code [n_codes] int64: counted rows (NUM_MEASUREMENTS);
 *   rank [n_codes] int32: the position of the code among the ELIGIBLE codes (at least one row and at least
 *     min_patient_count patients) in (patients descending, code ascending) order, -1 for a code that is not eligible;
 *   selected [n_codes] uint8: rank >= 0 && (top_k < 0 || rank < top_k) -- a negative top_k means no cut, a tie at the
 *     cut goes to the smaller code;
 *   out_rows [<= n] int32: the kept rows in ASCENDING order -- MMG_SEL_ROWS_ALL: every counted row of a selected code;
 *     MMG_SEL_ROWS_FIRST: of each (patient, code) pair of a selected code the row with the smallest index;
 *   *n_out (HOST): their number -- this call waits for the stream (as mmg_lab_aggregate does: the count sizes the
 *     caller's view of out_rows), so it cannot be captured.
 * Limits: 0 <= n < 2^31 (n = 0 is valid), 1 <= n_patients < 2^31, 1 <= n_codes < 2^31 -- NOT capped at
 * MMG_PREP_MAX_LABS: a raw vocabulary is cut down to that by this call -- and n_codes * n_patients + 1 < 2^63.  Every
 * argument is checked on the host before anything is enqueued (MMG_E_ARG; a short workspace MMG_E_WS).  Integer work,
 * no atomics on the data path, no memset node: every output is exact and bitwise reproducible.
 * ------------------------------------------------------------------------------------- */
#define MMG_SEL_ROWS_ALL 0
#define MMG_SEL_ROWS_FIRST 1
size_t mmg_code_select_ws_bytes(int64_t n, int64_t n_codes);
int mmg_code_select(const int64_t* code, const int64_t* patient, const uint8_t* valid, int64_t n, int64_t n_patients,
                    int64_t n_codes, int64_t min_patient_count, int64_t top_k, int rows_mode,
                    int64_t* n_patients_per_code, int64_t* n_rows_per_code, int32_t* rank, uint8_t* selected,
                    int32_t* out_rows, int64_t* n_out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Embedding maps (src/advanced_visualizations.py create_embedding_visualizations, src/visualize.py plot_embeddings_umap
 * with visualization.dim_reduction = "pca"; mmgnn/embed.py, csrc/pca.hip): the arithmetic over all rows of a PCA of
 * fp32 node embeddings and of the density grid of the projected patients.  X is fp32 [n, D] with row stride
 * ld_x >= D (elements); D is a multiple of 4 in [4, 256].
 *   mmg_centered_gram: mean_out (device, fp64 [D]) = the column means (fp64 sums, divided by n once); gram_out (device,
 *     fp64 [D * D]) = S = sum_i (x_i - mean)(x_i - mean)^T, centred in fp64 from the fp32 input (two passes over X, never
 *     X^T X - n mean mean^T), products and sums in fp64 (v_mfma_f64_16x16x4_f64).  One triangle is computed and
 *     mirrored: S is exactly symmetric.  2 <= n < 2^31.  Workgroups leave partial slabs in ws, summed in a fixed order.
 *   mmg_project_rows: out[i * ld_out + c] = scale[c] * sum_d (x_id - mean[d]) * comps[c * D + d] for c < k, the sum in
 *     fp64, rounded once to fp32; scale NULL = 1.  mean, comps, scale are DEVICE arrays (fp64 [D], [k * D], [k]).
 *     1 <= k <= 8, ld_out >= k, 1 <= n < 2^31.  One read of X.
 *   mmg_grid2d: numpy.histogram2d of the points (Y[i * ld_y], Y[i * ld_y + 1]) over explicit edges ex (DEVICE, fp64
 *     [gx + 1]) and ey ([gy + 1]), ascending: bins are half open, the last edge is inclusive, a point outside the edges
 *     or with a NaN coordinate is counted nowhere; the fp32 coordinate is widened exactly and compared with the edges.
 *     count[bx * gy + by] (device, int64 [gx * gy]) = the points of the cell, wsum = the sum of w[i] (int32, nullable;
 *     wsum may then be null) over them.  Both are zeroed by a kernel first.  1 <= gx, gy <= 256, 0 <= n < 2^31.
 *     Integer atomics only: the result does not depend on their order.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; mmg_centered_gram's workspace
 * MMG_E_WS); mmg_project_rows and mmg_grid2d need no workspace today (their *_ws_bytes is 0 and ws may be NULL).  No call
 * synchronises with the host, allocates, uses a memset node or a floating-point atomic; the order of every fp64 sum is
 * fixed by n and D: bitwise reproducible from run to run and eager against a replayed hipGraph.
 * ------------------------------------------------------------------------------------- */
size_t mmg_centered_gram_ws_bytes(int64_t n, int D);          /* 0 for an unsupported shape */
int mmg_centered_gram(const float* X, int64_t n, int D, int64_t ld_x, double* mean_out, double* gram_out, void* ws,
                      size_t ws_bytes, void* stream);
size_t mmg_project_rows_ws_bytes(int64_t n, int D, int k);
int mmg_project_rows(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* comps,
                     const double* scale, int k, float* out, int64_t ld_out, void* ws, size_t ws_bytes, void* stream);
size_t mmg_grid2d_ws_bytes(int64_t n, int gx, int gy);
int mmg_grid2d(const float* Y, int64_t ld_y, const int32_t* w, int64_t n, const double* ex, const double* ey, int gx,
               int gy, int64_t* count, int64_t* wsum, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exact t-SNE (src/advanced_visualizations.py create_embedding_visualizations -> sklearn.manifold.TSNE; mmgnn/embed.py
 * tsne, csrc/tsne.hip): the O(n^2) algorithm of TSNE(method="exact") with 2 map components.  X is fp32 [n, D] with row
 * stride ld_x >= D, D a multiple of 4 in [4, 256], 4 <= n <= MMG_TSNE_MAX_N.  A is ONE caller-owned fp32 n x n buffer
 * with row stride ld_a >= n (the padding is never written): the squared distances, then the joint probabilities, in
 * place.
 *   mmg_tsne_sqdist: A[i][j] = sum_d (x_id - x_jd)^2, the difference form in fp64 from the widened fp32 inputs (never
 *     the Gram form), columns in ascending order, rounded once to fp32.  The upper triangle is computed and mirrored: A
 *     is exactly symmetric and A[i][i] = 0.
 *   mmg_tsne_joint_p: sklearn's _binary_search_perplexity per row, in fp64 on the widened distances: beta = 1, at most
 *     100 steps; p_j = exp(-beta d_ij), p_i = 0; s = sum p (1e-8 if 0); H = log s + beta (sum d_ij p_j) / s; stop when
 *     |H - log(perplexity)| <= 1e-5, else double / halve beta while the far bound is infinite, else bisect.  The
 *     conditional row p / s, rounded to fp32, overwrites row i.  Then in place P_ij = max((double)(C_ij + C_ji) / S,
 *     eps) rounded to fp32, the sum C_ij + C_ji in fp32, S = max(sum_ij (C_ij + C_ji), eps) in fp64, eps = 2^-52; the
 *     diagonal is 0 and P is exactly symmetric.  beta_out (device, fp64 [n]) = the beta of the row that was written,
 *     steps_out (device, int32 [n]) = the number of evaluations of H (1 .. 100).  0 < perplexity < n.
 *   mmg_tsne_step: one iteration of sklearn's _gradient_descent on _kl_divergence, all in fp64; Y, U (the update) and
 *     G (the gains) are device fp64 [n, 2].  num_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} num_ij;
 *     Q_ij = max(num_ij / Z, eps), Pe_ij = exaggeration * (double)A_ij; grad_i = 4 sum_j (Pe_ij - Q_ij) num_ij
 *     (y_i - y_j); with want_kl, KL = sum_{i != j} Pe_ij log(max(Pe_ij, eps) / Q_ij).  Then inc = U grad < 0;
 *     gain = max(inc ? G + 0.2 : 0.8 G, min_gain); g = grad gain; and with update != 0: G = gain,
 *     U = momentum U - learning_rate g, Y += U -- every product and sum of this update rounded on its own (no fused
 *     multiply-add): bit-equal to numpy.  stats_out (device, fp64 [3]) = (KL or NaN, sum g^2, Z); grad_out (device,
 *     fp64 [n, 2], nullable) = the gradient before the gains.  With update = 0 only stats_out and grad_out are written.
 *     Three kernels: Z (a pass over Y alone), the gradient (one read of A; Y staged through LDS in tiles of
 *     MMG_TSNE_TILE points), the update.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short workspace MMG_E_WS;
 * mmg_tsne_sqdist needs none today: its *_ws_bytes is 0 and ws may be NULL).  No call synchronises with the host,
 * allocates, uses a memset node or a floating-point atomic; the order of every fp64 sum is fixed by n and D (a row's
 * sums are reduced over MMG_TSNE_SEARCH_WIDTH threads): bitwise reproducible from run to run and eager against a
 * replayed hipGraph.
 * ------------------------------------------------------------------------------------- */
#define MMG_TSNE_MAX_N 16384
#define MMG_TSNE_TILE 512
#define MMG_TSNE_SEARCH_WIDTH 256
size_t mmg_tsne_sqdist_ws_bytes(int64_t n, int D);
int mmg_tsne_sqdist(const float* X, int64_t n, int D, int64_t ld_x, float* A, int64_t ld_a, void* ws, size_t ws_bytes,
                    void* stream);
size_t mmg_tsne_joint_p_ws_bytes(int64_t n);                  /* 0 for an unsupported shape */
int mmg_tsne_joint_p(float* A, int64_t n, int64_t ld_a, double perplexity, double* beta_out, int32_t* steps_out, void* ws,
                     size_t ws_bytes, void* stream);
size_t mmg_tsne_step_ws_bytes(int64_t n);                     /* 0 for an unsupported shape */
int mmg_tsne_step(const float* A, int64_t n, int64_t ld_a, double exaggeration, double* Y, double* U, double* G,
                  double momentum, double learning_rate, double min_gain, int want_kl, double* stats_out, double* grad_out,
                  int update, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device graph build (src/graph_build.py NodeIndexer :34-97, :163-173, create_patient_*_edges :476-586, the flip(0)
 * reverse relations :222; mmgnn/graph_build.py build_graph_from_events, csrc/graph.hip): node indices in first-seen
 * order and one edge per event row whose two ids are known, from device arrays of CODES (int64, one code per key: the
 * caller factorises after the key rule).  A code outside its range means the row is ignored; it is never used as an
 * address.
 *   mmg_first_seen_index: the rows with a code in [0, n_codes) and valid[e] != 0 (valid uint8, nullable = every row)
 *     are the COUNTED rows.  index_of_code [n_codes] int32: the position of code c when the distinct codes are listed in
 *     the order of their first counted row (NodeIndexer.add order = Series.unique() order), -1 for a code without a
 *     counted row;  code_of_index int64, the inverse: min(n, n_codes) entries, the first *n_nodes are written;
 *     *n_nodes (HOST): the number of codes seen.
 *   mmg_edge_build: row e is KEPT when patient[e] is in [0, n_patient_codes), item[e] in [0, n_item_codes) and both
 *     patient_index[patient[e]] and item_index[item[e]] are >= 0 (int32 tables as mmg_first_seen_index writes them).
 *     The kept rows are compacted in ASCENDING row order; for the k-th of them fwd[0 * ld + k] = the patient index,
 *     fwd[1 * ld + k] = the item index (int64, ld >= n), rev (nullable) the same with the two rows swapped -- flip(0) --
 *     and attr[k] (fp32, nullable; needs value) = (float)value[e], ONE round-to-nearest-even from fp64 as
 *     astype(np.float32) does; a NaN value keeps its row.  A repeated (patient, item) pair gives one edge per row.
 *     fwd and rev hold 2 * ld entries, attr n; only the first *n_edges columns are written.
 *     *n_edges (HOST): the number of kept rows.
 * Both calls wait for the stream before they write the host count (as mmg_code_select does for n_out: the count sizes
 * the caller's views), so they cannot be captured.  Limits: 0 <= n < 2^31 (n = 0 is valid), 1 <= n_codes,
 * n_patient_codes, n_item_codes < 2^31.  Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a
 * short workspace MMG_E_WS).  Integer work: flags, an exclusive scan and a scatter that writes every output once; the
 * first row of a code is an integer atomicMin over a table a kernel filled (no memset node), whose result does not
 * depend on the order.  Every output is exact and bitwise equal from call to call.
 * ------------------------------------------------------------------------------------- */
size_t mmg_first_seen_index_ws_bytes(int64_t n, int64_t n_codes);
int mmg_first_seen_index(const int64_t* code, const uint8_t* valid, int64_t n, int64_t n_codes, int32_t* index_of_code,
                         int64_t* code_of_index, int64_t* n_nodes, void* ws, size_t ws_bytes, void* stream);
size_t mmg_edge_build_ws_bytes(int64_t n);
int mmg_edge_build(const int64_t* patient, const int64_t* item, const double* value, int64_t n,
                   const int32_t* patient_index, int64_t n_patient_codes, const int32_t* item_index,
                   int64_t n_item_codes, int64_t* fwd, int64_t* rev, int64_t ld, float* attr, int64_t* n_edges, void* ws,
                   size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_H */
