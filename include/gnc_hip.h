/*
 * gnc_hip.h -- C ABI of the MI355X (gfx950) message-passing engine that stands behind the
 * GraphNet forward hot path of alexisvannson/GraphNet_Classifier.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own:
 * its narrowest seam is the module-level Python name `scatter_sum` bound at import
 * (reference models/GNN.py:4-21, where an optional C++ extension or an `index_add_` fallback
 * is chosen) plus the `torch.nn.Module` forward methods of `MLP`, `EdgeProcessor`,
 * `NodeProcessor`, `GraphProcessor` and `GraphNet`.  Each entry point below names the
 * reference line(s) whose work it replaces.  A maintainer of the reference binds these with
 * `ctypes` (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked host;
 *   - `stream` is a `hipStream_t` passed as `void*`; nothing here synchronises the stream,
 *     allocates, or frees: outputs and workspaces are caller-allocated (the Python side uses
 *     torch's caching allocator) so calls can be captured into a hipGraph;
 *   - return value: 0 = GNC_OK, negative = error (see enum); `gnc_last_error_string()` gives
 *     a thread-local description of the last failure on the calling thread;
 *   - matrices are row-major fp32; `ld*` are leading dimensions in ELEMENTS;
 *   - indices are int32 inside the engine; the int64 `edge_index` of the reference
 *     (utils/dataloader.py:51) is narrowed once, by `gnc_csr_build`.
 */
#ifndef GNC_HIP_H
#define GNC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNC_ABI_VERSION 20

enum {
  GNC_OK = 0,
  GNC_ERR_INVALID_ARGUMENT = -1, /* null pointer, negative size, misaligned buffer ...      */
  GNC_ERR_UNSUPPORTED = -2,      /* shape outside what the kernels are instantiated for      */
  GNC_ERR_WORKSPACE = -3,        /* workspace smaller than gnc_*_workspace_bytes() reports   */
  GNC_ERR_HIP = -4               /* a HIP runtime call or a kernel launch failed             */
};

#define GNC_MAX_SEGMENTS 4 /* concat segments feeding the first Linear of an MLP */
#define GNC_MAX_LINEAR 8   /* Linear layers in one MLP (hidden_layers + 1)       */

enum { GNC_ACT_RELU = 0, GNC_ACT_IDENTITY = 1, GNC_ACT_TANH = 2, GNC_ACT_SIGMOID = 3,
       GNC_ACT_SILU = 4, GNC_ACT_GELU = 5, GNC_ACT_LEAKY_RELU = 6, GNC_ACT_ELU = 7 };

/* ---- diagnostics --------------------------------------------------------------------- */
int gnc_abi_version(void);
const char* gnc_last_error_string(void);
/* Name of the device code object target this library was built for ("gfx950"). */
const char* gnc_target_arch(void);

/* ---- topology: edge list -> destination-sorted CSR ------------------------------------
 * Replaces nothing the reference does explicitly: the reference re-derives "who sends to
 * node v" inside every `index_add_` (models/GNN.py:18-20).  Here the destination column of
 * `edge_index` (models/GNN.py:98 `_, col = edge_index`) is sorted once per topology.
 *
 *   index   [E] int64   destination (or source) node id per edge, any order
 *   rowptr  [N+1] int32 out: edges of node v are sorted positions rowptr[v] .. rowptr[v+1]-1
 *   perm    [E] int32   out: perm[k] = ORIGINAL edge id at sorted position k.  The sort is
 *                       stable, so inside a segment edges keep their original order and the
 *                       per-destination summation order equals the reference's edge order.
 *   status  [1] int32   out: 0, or 1 if any index was outside [0, N) (such edges are dropped
 *                       instead of faulting; the reference raises IndexError there)
 */
size_t gnc_csr_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int gnc_csr_build(const int64_t* index, int64_t num_edges, int64_t num_nodes,
                  int32_t* rowptr, int32_t* perm, int32_t* status,
                  void* workspace, size_t workspace_bytes, void* stream);

/* out[k] = (int32) src[perm[k]]   -- narrows and reorders an int64 edge_index row. */
int gnc_permute_index_i64_i32(const int64_t* src, const int32_t* perm, int64_t n, int32_t* out, void* stream);
/* Same, and validates on the way: a value outside [0, num_nodes) sets *status (device int32, caller zero-fills)
 * to 1 and is stored as 0, so that nothing downstream can index out of range before the host has looked at
 * the flag (models/GNN.py:18-20: `index_add_` raises IndexError for such an id). */
int gnc_permute_index_checked_i64_i32(const int64_t* src, const int32_t* perm, int64_t n, int64_t num_nodes, int32_t* out,
                                      int32_t* status, void* stream);

/* ---- topology of a graph-ordered batch in one call (ABI 17) --------------------------------
 * Everything `GraphNet.forward` needs of `edge_index` (models/GNN.py:98 `_, col = edge_index`, the x[row] / x[col]
 * gathers of MetaLayer at :215) from ONE call: the destination CSR (rowptr, perm: the stable sort of gnc_csr_build) and
 * both endpoint vectors narrowed to int32 and reordered by it (src_sorted[k] = src[perm[k]], dst_sorted[k] = dst[perm[k]];
 * what gnc_permute_index_checked_i64_i32 / gnc_permute_index_i64_i32 give).  Batches of small graphs whose edges are
 * contiguous in edge_index (the reference's loader yields one self-contained graph per item, utils/dataloader.py:33-53;
 * graphs of at most 2048 edges) are sorted range by range in LDS without a global radix sort;
 * any other edge list raises status[2] ON THE DEVICE and is sorted by a general stable LSD radix sort: ONE kernel that
 * is enqueued behind it and returns at once unless the flag is set - so the call never synchronises and can be
 * captured (gated_fallback = 1).  A caller that reads the flags back anyway may pass gated_fallback = 0 (smaller
 * workspace) and run gnc_csr_build + the permutes itself when status[2] is set.
 *
 *   src, dst      [E] int64 (index_bytes = 8) or int32 (index_bytes = 4) node ids; src may be NULL: then only rowptr and
 *                 perm are produced (src_sorted / dst_sorted ignored)
 *   status [3]    out: [0] = a destination outside [0, N), [1] = a source outside [0, N) (such ids are replaced by 0:
 *                 nothing downstream can index out of range; models/GNN.py:18-20 raises IndexError there),
 *                 [2] = 1: the LDS path could not take this edge list (informational when gated_fallback = 1: the general
 *                 path - one gated launch whose passes meet at a grid barrier - has sorted it); 2: that barrier timed out
 *                 (5 s; the outputs are invalid, status[0] is raised as well so that every validity check fails)
 */
size_t gnc_topology_workspace_bytes(int64_t num_nodes, int64_t num_edges, int32_t gated_fallback);
int gnc_topology_build(const void* src, const void* dst, int32_t index_bytes, int64_t num_edges, int64_t num_nodes,
                       int32_t* rowptr, int32_t* perm, int32_t* src_sorted, int32_t* dst_sorted, int32_t* status,
                       void* workspace, size_t workspace_bytes, int32_t gated_fallback, void* stream);

/* ---- K1: scatter-sum neighbourhood aggregation ------------------------------------------
 * Replaces `scatter_sum(edge_attr, col, dim=0)` (models/GNN.py:99 -> :11-21):
 *   out[v, :] = sum over sorted positions k in [rowptr[v], rowptr[v+1]) of src[row(k), :]
 * with row(k) = perm[k], or k itself when `perm` is NULL (messages already stored in
 * destination-sorted order).  No atomics: each destination is summed by one lane group in
 * ascending k, so the result is bitwise reproducible and every out row is written
 * (zero for a node without in-edges), no memset needed.
 */
int gnc_scatter_sum_csr_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* perm,
                            int64_t num_nodes, int64_t num_edges, int32_t feat_dim,
                            float* out, int64_t ld_out, void* stream);

/* ---- K2: row gather -----------------------------------------------------------------------
 * Replaces `x[row]`, `x[col]` of PyG MetaLayer.forward (called at models/GNN.py:215) and is the
 * backward of K1:  out[r, :] = table[index[r], :].
 */
int gnc_gather_rows_f32(const float* table, int64_t ld_table, const int32_t* index, int64_t num_rows,
                        int32_t feat_dim, float* out, int64_t ld_out, void* stream);
/* out[r, :] = table[index[r], :] + addend[r, :]: the gradient of an edge latent that feeds both the aggregation
 * (backward of K1 = this gather) and the next block (addend), formed in one pass. */
int gnc_gather_rows_add_f32(const float* table, int64_t ld_table, const int32_t* index, const float* addend,
                            int64_t ld_addend, int64_t num_rows, int32_t feat_dim, float* out, int64_t ld_out, void* stream);

/* ---- K6: edge features ------------------------------------------------------------------
 * Replaces models/GNN.py:299-302:  rel = pos[dst[e]] - pos[src[e]];  out[e] = [rel, sum|rel|].
 * pos is [N, space_dim]; out is [E, ld_out] with ld_out >= space_dim + 1; columns past the
 * features are written as zero (ld_out = 4 for space_dim = 2 gives 16-B rows the MLP kernels can
 * load with one vector instruction).
 */
int gnc_edge_features_f32(const float* pos, int32_t space_dim, const int32_t* src, const int32_t* dst,
                          int64_t num_edges, float* out, int64_t ld_out, void* stream);

/* ABI 19.  Deferred validation of a topology (status flags still on the device when the forward is enqueued): overwrite the
 * `count` contiguous floats of `out` with NaN when any of flags[0 .. nflags) is non-zero; one launch that returns at once
 * otherwise.  Keeps a forward on an edge_index with out-of-range ids (models/GNN.py:18-20 raises IndexError there) from
 * yielding plausible numbers before the host has read the flags.  nflags <= 16. */
int gnc_poison_if_flagged_f32(float* out, int64_t count, const int32_t* flags, int32_t nflags, void* stream);

/* ---- K4: fused MLP ----------------------------------------------------------------------
 * Replaces `MLP.forward` (models/MLP.py:45-47 over the Sequential built at :24-37) together
 * with the `torch.cat` in front of it and the residual add behind it in the processors
 * (models/GNN.py:58-62 and :100-102):
 *
 *   in[r]  = concat over segments s of  seg[s].ptr[ row_s(r), 0:width_s ]      (never materialised)
 *            row_s(r) = seg[s].index[r] if index != NULL else r                 (fused gather, K2+K3)
 *   h      = act(in  W0^T + b0);  h = act(h Wl^T + bl) ...;  y = h W_last^T + b_last
 *   y      = LayerNorm(y) * gamma + beta        if ln_gamma != NULL  (eps = ln_eps)
 *   out[r] = y + residual[r]                    if residual != NULL
 *
 * Weights are nn.Linear layout [out_dim, in_dim] row-major (state-dict tensors are passed
 * as they are).  fp32 in, fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 out.
 * Limits: hidden widths and out width <= 256, 1 <= num_linear <= GNC_MAX_LINEAR, all
 * hidden layers the same width (true by construction in models/MLP.py:24-27).
 * in_dim[0] is the summed width of the GNC_SEG_MATMUL segments.  When `residual` is the table of
 * the LAST listed segment (no index, same ld, width == out width <= 64) the kernel takes the
 * residual from the rows it has already staged instead of reading them again.  num_linear == 1 is a plain
 * (optionally LayerNorm-ed) projection.
 *
 * W-split.  W0 [x_src | x_dst | e]^T = Ws x[src] + Wd x[dst] + We e: the node-side products can
 * be formed once per NODE (two num_linear == 1 launches over [N, Dn]) and merely gathered and
 * added per EDGE (GNC_SEG_ADD segments), which removes 2/3 of the first Linear's per-edge MFMA
 * work of models/GNN.py:58-61.  ld_weight lets We be passed as a column slice of W0.
 */
enum { GNC_SEG_MATMUL = 0, /* columns of the virtual concat: multiplied by their slice of weight[0]      */
       GNC_SEG_ADD = 1     /* rows already projected to the hidden width: added to the first Linear's
                              pre-activation (width must equal out_dim[0]); see "W-split" below       */ };

typedef struct gnc_mlp_segment {
  const float* ptr;     /* [*, ld] table                                   */
  const int32_t* index; /* NULL, or [rows] row ids into the table          */
  int32_t width;        /* columns taken from the table                    */
  int32_t ld;           /* leading dimension of the table (elements)       */
  int32_t mode;         /* GNC_SEG_MATMUL | GNC_SEG_ADD                    */
  int32_t wcol;         /* MATMUL: first column of weight[0] this segment multiplies (segments may be
                           listed, i.e. staged, in any order; the concat order lives here)          */
  int64_t table_rows;   /* rows of the table behind ptr = bound of the ids in `index`; REQUIRED (> 0) whenever
                           index != NULL.  Every kernel variant treats an id outside [0, table_rows) the same
                           way: the row reads as zeros, never a fault (tables below 4 GiB through the hardware
                           bounds check of a buffer window, larger ones by an explicit compare).
                           Ignored when index == NULL */
} gnc_mlp_segment_t;

typedef struct gnc_mlp_desc {
  int32_t num_segments;
  int32_t num_linear;
  int32_t activation;   /* GNC_ACT_*                                       */
  float act_param;      /* negative slope / alpha for LEAKY_RELU / ELU     */
  gnc_mlp_segment_t seg[GNC_MAX_SEGMENTS];
  const float* weight[GNC_MAX_LINEAR]; /* [out_dim[l], in_dim[l]]          */
  int32_t ld_weight[GNC_MAX_LINEAR];   /* row stride of weight[l]; 0 = in_dim[l] (contiguous) */
  const float* bias[GNC_MAX_LINEAR];   /* [out_dim[l]] or NULL             */
  int32_t in_dim[GNC_MAX_LINEAR];
  int32_t out_dim[GNC_MAX_LINEAR];
  const float* ln_gamma; /* NULL = no LayerNorm                            */
  const float* ln_beta;
  float ln_eps;
  const float* residual; /* NULL, or [rows, ld_residual]                   */
  int32_t ld_residual;
  float* out;            /* [rows, ld_out]                                 */
  int32_t ld_out;
  int64_t rows;
  /* Fused aggregation epilogue ("CSR-ordered segmented-sum epilogue"); all NULL / 0 = off.
   * With agg_out set, the launch ALSO forms agg_out[v, :] = sum of the output rows r with agg_index[r] == v,
   * added in ascending r starting from 0.0 - bit for bit what gnc_scatter_sum_csr_f32 gives on `out` -
   * for every destination whose rows lie inside ONE wave's contiguous row range.  Contract:
   *   - agg_index [rows] int32 is non-decreasing (rows are in destination-CSR order);
   *   - destinations without rows are not written by the kernel: gnc_agg_fixup_f32 zero-fills them;
   *   - destinations cut by a range boundary are not written either: the kernel lists them (and -1 for
   *     idle waves) in agg_fix [gnc_mlp_agg_fix_len()] int32, and gnc_agg_fixup_f32 recomputes exactly
   *     those rows from `out` through the row pointers afterwards (same stream).
   * Served by the weights-resident kernel (widths <= 64), the 32-row streaming kernel (65..128) and the 16-row
   * streaming kernel (129..256, num_linear > 1): ask gnc_mlp_agg_supported(); gnc_mlp_forward_f32 returns
   * GNC_ERR_UNSUPPORTED otherwise.  Not offered for small batches at 65..128 features (gnc_mlp_small_batch_supported):
   * there gnc_scatter_sum_csr_f32 on the output rows is the cheaper route. */
  float* agg_out;           /* [*, ld_agg] or NULL */
  int32_t ld_agg;
  const int32_t* agg_index; /* [rows] destination of each output row */
  int32_t* agg_fix;         /* [gnc_mlp_agg_fix_len()] destinations left to gnc_agg_fixup_f32 */
  /* ABI 16, training forward: save_act[l] (l < num_linear - 1) = NULL, or [rows, out_dim[l]] contiguous: the launch
   * also writes the post-activation output of Linear l (what torch.autograd keeps for the backward of
   * models/MLP.py:45-47), so that gnc_mlp_backward_f32 can read it (act_given) instead of recomputing the forward of
   * every tile.  All of them or none; only where gnc_mlp_save_act_supported() says so. */
  float* save_act[GNC_MAX_LINEAR];
  /* ABI 19, K6 as the prologue of the edge encoder (models/GNN.py:299-302 feeding :306).  ef_pos = NULL: off.
   * With ef_pos set, the rows of segment 0 - the only segment: MATMUL, index NULL, width = ef_space_dim + 1, its ptr / ld
   * ignored - are COMPUTED by the launch instead of read:
   *   row r = [ pos[ef_dst[r]] - pos[ef_src[r]] , sum_d |pos[ef_dst[r]][d] - pos[ef_src[r]][d]| ]
   * (the differences summed in dimension order starting from the first: bit for bit what gnc_edge_features_f32 stores), so
   * the [rows, space_dim + 1] table never exists in HBM.  pos [ef_nodes, ef_space_dim] contiguous; an id outside
   * [0, ef_nodes) reads as a zero position, never a fault.  Inference only (no save_act, no agg_out); served where
   * gnc_mlp_edge_features_supported() says so (the weights-resident kernel, ef_space_dim = 2, hidden widths <= 64, a batch
   * above the small-batch limit); gnc_mlp_forward_f32 returns GNC_ERR_UNSUPPORTED otherwise and the caller runs
   * gnc_edge_features_f32 + a plain segment. */
  const float* ef_pos;
  const int32_t* ef_src;
  const int32_t* ef_dst;
  int64_t ef_nodes;
  int32_t ef_space_dim;
} gnc_mlp_desc_t;

/* 0 if gnc_mlp_forward_f32 can run this description, GNC_ERR_UNSUPPORTED otherwise
 * (pointers are not inspected, only the shape fields). */
/* sizeof(gnc_mlp_desc_t) as compiled into the library, for binding cross-checks. */
size_t gnc_sizeof_mlp_desc(void);
int gnc_mlp_supported(const gnc_mlp_desc_t* desc /* host */);
/* The kernel family is chosen by one walk (forward_chain in mlp_fused.hip; the table in DESIGN.md, K4); the save_act,
 * operands_in_place and small_batch queries below answer as routed by it. */
int gnc_mlp_forward_f32(const gnc_mlp_desc_t* desc /* host */, void* stream);
/* fused aggregation epilogue: 0 if this description can run with agg_out set (shape fields only) */
int gnc_mlp_agg_supported(const gnc_mlp_desc_t* desc /* host */);
int gnc_mlp_agg_fix_len(void); /* entries of agg_fix (2 per wave of the persistent grid) */
/* Aggregate-only launch: the description of an agg_out launch whose output rows nobody reads afterwards (the last GN block's
 * edge processor in inference).  agg_out and agg_fix are formed exactly as gnc_mlp_forward_f32 forms them, bit for bit, but
 * `out` [rows, ld_out] is written ONLY at the rows whose destination is listed in agg_fix - the rows gnc_agg_fixup_f32 reads;
 * every other row of `out` is left as it was.  Run gnc_agg_fixup_f32 afterwards as for the storing launch.
 * gnc_mlp_agg_only_supported() answers from the shape fields (GNC_ERR_UNSUPPORTED: use gnc_mlp_forward_f32): served for the
 * 64-wide W-split edge processor (1 MATMUL + 2 ADD segments, residual = the MATMUL segment, three Linear layers, LayerNorm,
 * 16-B aligned output) wherever gnc_mlp_agg_supported() serves it, without save_act. */
int gnc_mlp_agg_only_supported(const gnc_mlp_desc_t* desc /* host */);
int gnc_mlp_forward_agg_only_f32(const gnc_mlp_desc_t* desc /* host */, void* stream);
/* ABI 19: 0 if the kernel that gnc_mlp_forward_f32 picks for this description reads its operands where they lie: weight
 * matrices of any row stride / alignment (the [H, 3] matrix of nn.Linear(3, H), models/GNN.py:251-256) and a contiguous
 * [rows, 3] table as the only segment (the node features of models/GNN.py:305) - no zero-padded copies needed.  Every other
 * kernel reads rows of 16-B pieces (tables and weights 16-B aligned, leading dimensions % 4 == 0). */
int gnc_mlp_operands_in_place_supported(const gnc_mlp_desc_t* desc /* host */);
/* ABI 19: 0 if gnc_mlp_forward_f32 serves this description with ef_pos set (pointer fields: alignment tests only) */
int gnc_mlp_edge_features_supported(const gnc_mlp_desc_t* desc /* host */);
/* ABI 18.  0 if the small-batch kernel (one 16-row tile per workgroup, the waves split the output features; rows up to
 * 128 x the number of CUs, widths 65..128, ReLU) serves this description EXACTLY AS GIVEN: it is the only kernel that reads
 * tables and weights whose rows are not 16-B pieces (the reference's [N, 3] inputs and nn.Linear(3, H) weights,
 * models/GNN.py:251-253) in place; for every other launch the caller hands over zero-padded copies.  The reference's own
 * regime (one graph per call: main.py:60, utils/train_model.py:35-45, utils/inference.py:59) runs on it. */
int gnc_mlp_small_batch_supported(const gnc_mlp_desc_t* desc /* host */);
/* ABI 18: out = a W[:, 0:dn] + b W[:, dn:2 dn] for W [hidden, ld_w] as nn.Linear holds it (read transposed, no copy): the
 * node-side gradient of the W-split first Linear (dx = d(ps) Ws + d(pd) Wd) in one launch for a small batch (hidden = dn = 128,
 * 16-B aligned rows); GNC_ERR_UNSUPPORTED otherwise, nothing launched. */
int gnc_mlp_projection_t2_f32(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t rows, const float* w, int64_t ld_w,
                              int32_t hidden, int32_t dn, float* out, int64_t ld_out, void* stream);
int64_t gnc_mlp_small_batch_max_rows(void); /* the row limit of the small-batch forward kernel (128 x CUs unless overridden) */
/* ABI 18: out_a = x wa^T and out_b = x wb^T (no bias) over the same row-ordered x [rows, in_dim] in ONE launch: the two
 * node-side products of the W-split first Linear (models/GNN.py:58-61 formed once per node).  Two shapes: the small-batch
 * projection (in_dim = out_dim = 128, rows within the small-batch limit, 16-B aligned rows, ld_wa == ld_wb) and - since ABI 19 -
 * a batch above that limit at in_dim <= 64, out_dim 36..64 (a multiple of 4) on the weights-resident kernel (rows read and
 * staged once, both matrices resident in LDS, read where they lie whatever their row stride).  GNC_ERR_UNSUPPORTED otherwise,
 * nothing launched - issue two gnc_mlp_forward_f32 launches then. */
int gnc_mlp_dual_projection_f32(const float* x, int64_t ld_x, int64_t rows, const float* wa, int64_t ld_wa, const float* wb,
                                int64_t ld_wb, int32_t in_dim, int32_t out_dim, float* out_a, float* out_b, int64_t ld_out,
                                void* stream);
/* 0 if gnc_mlp_forward_f32 can run this description with save_act set (every kernel but the generic fallback: ReLU, hidden
 * widths that are multiples of 4 and at most 256, aligned tables), GNC_ERR_UNSUPPORTED otherwise (shape fields only) */
int gnc_mlp_save_act_supported(const gnc_mlp_desc_t* desc /* host */);
/* out[v, :] = sum over k in [rowptr[v], rowptr[v+1]) of src[k, :] (ascending k) for the n_fix destinations
 * v = fix[j] (entries < 0 or >= num_nodes are skipped; duplicates are harmless), and out[v, :] = 0 for every
 * destination v < num_nodes without rows: together with the epilogue every row of `out` is then defined. */
int gnc_agg_fixup_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* fix, int32_t n_fix,
                      int64_t num_nodes, int32_t feat_dim, float* out, int64_t ld_out, void* stream);

/* ---- K8: backward of the fused MLP ---------------------------------------------------------
 * Replaces what PyTorch's autograd does for `loss.backward()` (utils/train_model.py:41) through
 * models/MLP.py:45-47 and the concat/residual around it.  Two kernels:
 *
 * gnc_mlp_backward_f32: given the forward description `fwd` (its `out` field is ignored) and
 *   grad_out = dL/d(out) [rows, out_dim], recomputes the forward per 32-row tile - or, with act_given (ABI 16), reads the
 *   post-activations the training forward saved (gnc_mlp_desc_t.save_act) and recomputes only the last Linear for the
 *   LayerNorm statistics - and writes
 *     act[l]  [rows, out_dim[l]]  post-activation output of Linear l, l < num_linear-1 (input of Linear l+1); an INPUT
 *                                 with act_given
 *     dz[l]   [rows, out_dim[l]]  dL/d(pre-activation of Linear l); dz[num_linear-1] is dL/d(pre-LayerNorm y)
 *     dx      [rows, in_dim[0]]   dL/d(MATMUL part of the input concat), column order = wcol; NULL to skip
 *     yhat    [rows, out_dim]     normalised pre-affine output of the LayerNorm (required with LayerNorm):
 *                                 d beta = colsum(grad_out), d gamma = colsum(grad_out * yhat) -> gnc_colsum_pair_f32
 *   The gradient of an ADD segment's table rows is dz[0] itself (scatter it by the segment's index);
 *   the gradient of the residual is grad_out.  Weight gradients: dW_l = dz[l]^T (input of Linear l),
 *   db_l = column sums of dz[l] -> gnc_xty_f32.
 *   Supported: ReLU, 2 <= num_linear <= 7, tables 16-B aligned with ld % 4 == 0; widths <= 64 with every
 *   segment <= 64 columns and MATMUL segments listed before 0 or 2 ADD segments run with LDS-resident
 *   weights, other shapes up to width 128 stream the weights on 32-row tiles, widths 129..256 on 16-row tiles
 *   (v_mfma_f32_16x16x4_f32; both streaming forms need 16-B aligned weights, the 16-row one stated gather tables);
 *   gnc_mlp_backward_supported() answers from the shape fields alone.
 *
 * gnc_xty_f32: partial[w] = [ A^T B (M x K, row-major) | column sums of A (M) ] over the rows worker w
 *   streamed; sum the gnc_xty_partials_for(rows, M, K) rows it writes (fixed order => reproducible).  Both operands
 *   above 64 columns: M, K <= 256, one partial per WORKGROUP (the row tile is shared by the workgroup's waves, each
 *   row of A and B is read once per launch); otherwise M, K <= 128 and one partial per wave
 *   (= gnc_xty_partials(rows), which is also an upper bound of every count).
 * gnc_colsum_pair_f32: partial[w] = [ colsum(G) (width) | colsum(G * Y) (width) ], same partial count.
 */
typedef struct gnc_mlp_bwd_desc {
  gnc_mlp_desc_t fwd;
  const float* grad_out;
  int32_t ld_grad_out;
  float* act[GNC_MAX_LINEAR];
  float* dz[GNC_MAX_LINEAR];
  float* dx;
  int32_t ld_dx;
  float* yhat;
  int32_t dx_add_grad_out; /* 1: the LAST MATMUL segment is also the residual and out_dim equals its width: its dx
                              columns get grad_out added in the kernel (honoured by the weights-resident variant;
                              gnc_mlp_backward_dx_add_honoured() tells) */
  float* ln_partial;       /* NULL, or [gnc_mlp_backward_ln_partial_rows(fwd), 2 * out_dim]: row w receives
                              [ colsum(grad_out) | colsum(grad_out * yhat) ] over the rows wave w processed (sum the
                              rows in order: d beta, d gamma).  With it `yhat` is neither needed nor written and
                              gnc_colsum_pair_f32 is not needed: 3 x [rows, out_dim] of HBM traffic less per launch. */
  float* dw_partial[GNC_MAX_LINEAR]; /* all NULL, or for l < num_linear: [gnc_mlp_backward_fused_rows(fwd), M_l*K_l + M_l]
                              with M_l = out_dim[l], K_l = in_dim[l] (l = 0: the width of the MATMUL segment): row w
                              receives [ dW_l row-major | db_l ] over the rows wave w processed - the layout of
                              gnc_xty_f32, formed INSIDE the data kernel.  With it act[], dz[1..], yhat are neither
                              needed nor written (dz[0] still is when given); ln_partial is required with LayerNorm. */
  /* ABI 16: a gathered part of the output gradient.  When grad_gather is given, the gradient of output row r is
   *   (grad_out ? grad_out[r] : 0) + grad_gather[grad_gather_index[r]]
   * (table [grad_gather_rows, ld_grad_gather], first out_dim columns; an id outside the table contributes zeros).
   * This is the backward of the scatter-sum that consumed the rows (models/GNN.py:99: d agg[col[e]] / d e'[e] = I)
   * folded into the K8 launch: no [rows, out_dim] gather pass in front of it.  grad_out may then be NULL (the rows
   * had no other consumer).  Only kernels for which gnc_mlp_backward_grad_gather_honoured() returns 1 accept it.
   * grad_sum: device scratch [rows, ld_grad_sum >= out_dim] (16-B aligned, ld % 4 == 0), required when grad_out,
   * grad_gather and dx_add_grad_out are all given: the kernel parks the summed rows there for the residual path of
   * dx (contents undefined afterwards). */
  const float* grad_gather;
  int32_t ld_grad_gather;
  const int32_t* grad_gather_index;
  int64_t grad_gather_rows;
  float* grad_sum;
  int32_t ld_grad_sum;
  /* ABI 16: 1 = act[l] (l < num_linear - 1) are INPUTS: the post-activations the forward saved (gnc_mlp_desc_t.save_act,
   * contiguous [rows, out_dim[l]]); the kernel reads them instead of recomputing the forward of every tile.  Only where
   * gnc_mlp_backward_saved_act_honoured() returns 1 (the fused data + weight-gradient kernel: dw_partial given). */
  int32_t act_given;
  /* ABI 18: with act_given, fwd.save_act[l] carries the same pointers as act[l]: the shape queries that only take the forward
   * description (gnc_mlp_backward_ln_partial_rows, gnc_mlp_backward_dx_add_honoured, gnc_mlp_backward_supported) then answer
   * for the kernel that will run - small batches (rows <= 32 x CUs, widths 65..128) with saved activations run the column-split
   * (above that, at exactly 128 features, its register-resident variant)
   * data kernel (mlp_bwd_col16.hip): one ln_partial row per 16-row tile, grad_gather and dx_add_grad_out folded in. */
} gnc_mlp_bwd_desc_t;

size_t gnc_sizeof_mlp_bwd_desc(void);
/* The seven queries below all read the one routing decision gnc_mlp_backward_f32 itself launches by (bwd_route in
 * mlp_backward.hip; the table in DESIGN.md, K8).  Those that take only `fwd` answer as routed by it for a launch that
 * wants dx, with act_given where fwd.save_act[0] is set, on the split path (no dw_partial). */
int gnc_mlp_backward_supported(const gnc_mlp_desc_t* fwd /* host */);       /* 0: some data kernel is routed */
int gnc_mlp_backward_dx_add_honoured(const gnc_mlp_desc_t* fwd /* host */); /* 1: the routed kernel folds dx_add_grad_out */
/* ABI 18: 1 if the routed kernel is the small-batch data kernel, which reads the operands exactly as they lie: no 16-B-row
 * copies of [N, 3] inputs / nn.Linear(3, H) weights are needed in front of it */
int gnc_mlp_backward_small_batch_supported(const gnc_mlp_desc_t* fwd /* host */);
/* 1 if the kernel routed for desc (grad_gather*, dw_partial, dx and act_given filled in as for the call) gathers
 * desc->grad_gather in the launch, else 0: the caller gathers the rows itself (gnc_gather_rows_f32 / gnc_gather_rows_add_f32) */
int gnc_mlp_backward_grad_gather_honoured(const gnc_mlp_bwd_desc_t* desc /* host */);
/* 1 if the kernel routed for desc with act_given (act[], dw_partial and dx filled in as for the call) reads act[] */
int gnc_mlp_backward_saved_act_honoured(const gnc_mlp_bwd_desc_t* desc /* host */);
/* rows of `ln_partial` the routed kernel fills, 0 if it cannot form the LayerNorm sums in flight (it writes yhat) */
int gnc_mlp_backward_ln_partial_rows(const gnc_mlp_desc_t* fwd /* host */);
/* rows of `dw_partial[l]` (and then also of `ln_partial`) if a launch with dw_partial is routed to the fused data +
 * weight-gradient kernel, else 0 */
int gnc_mlp_backward_fused_rows(const gnc_mlp_desc_t* fwd /* host */);
int gnc_mlp_backward_f32(const gnc_mlp_bwd_desc_t* desc /* host */, void* stream);
int gnc_xty_partials(int64_t rows);
int gnc_xty_partials_for(int64_t rows, int32_t M, int32_t K);
int gnc_xty_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t rows, int32_t M, int32_t K,
                float* partial, int32_t num_partials, void* stream);
int gnc_colsum_pair_f32(const float* G, int64_t ldg, const float* Y, int64_t ldy, int64_t rows, int32_t width,
                        float* partial, int32_t num_partials, void* stream);
/* Fixed-order sum of per-wave partial rows written by the kernels above (and by dw_partial / ln_partial):
 * for j < M*K: dW[(j / K) * ld_dw + j % K] = sum_p partial[p * stride + j]; for j < M: db[j] = sum_p partial[p * stride + M*K + j]
 * (db may be NULL).  Lets a weight-gradient block land in its place inside a larger matrix without a PyTorch sum + copies. */
int gnc_reduce_partials_f32(const float* partial, int32_t num_partials, int32_t stride, int32_t M, int32_t K,
                            float* dW, int64_t ld_dw, float* db, void* stream);

/* ---- weight gradients of a small batch (ABI 18) ------------------------------------------------------------
 * The reference trains on one graph per step (utils/train_model.py:35-45): ~2000 rows per product.  gnc_xty_small_f32
 * forms SEVERAL products in ONE launch, without partial buffers or a reduction launch:
 *   kind 0:  dw[m, k] = sum over r of a[r, m] * b[r, k]   (dw [m, ld_dw]; any row stride, so a block of a wider matrix)
 *            db[m]    = sum over r of a[r, m]             (db may be NULL)
 *   kind 1:  dw[c]    = sum over r of a[r, c], c < m      (rows of per-tile partial sums -> one row; b, k, db unused)
 * Sums run in a fixed order (bitwise reproducible).  rows <= gnc_xty_small_max_rows() for every job. */
#define GNC_XTY_MAX_JOBS 8
typedef struct gnc_xty_job {
  const float* a;
  int64_t lda;
  const float* b;
  int64_t ldb;
  int64_t rows;
  int32_t m, k;
  float* dw;
  int64_t ld_dw;
  float* db;
  int32_t kind;
} gnc_xty_job_t;
int gnc_xty_small_max_rows(void);
int gnc_xty_small_f32(const gnc_xty_job_t* jobs /* host */, int32_t num_jobs, void* stream);

/* ---- backward of an MLP with an activation other than ReLU (ABI 17) ---------------------------------------
 * models/MLP.py:21 accepts any nn.<Name>; the reference's entry points only use ReLU, which the fused K8 kernels
 * above serve.  For the other activations of GNC_ACT_* the backward runs LAYER BY LAYER on this library: the
 * pre-activations are recomputed with single-Linear gnc_mlp_forward_f32 launches, these three row-wise / elementwise
 * kernels provide act, act' and the LayerNorm backward, the products da = dz W are single-Linear launches on the
 * transposed weights and the weight gradients come from gnc_xty_f32 / gnc_colsum_pair_f32.
 *   gnc_activation_f32           out = act(z)
 *   gnc_activation_backward_f32  grad_z = grad_act * act'(z)      (the derivative torch.autograd uses for nn.<Name>)
 *   gnc_layer_norm_backward_f32  for out = LayerNorm(y) * gamma + beta: grad_y and the normalised y_hat of every row
 *                                (d gamma = colsum(grad_out * y_hat), d beta = colsum(grad_out))
 */
int gnc_activation_f32(const float* z, int64_t ld_z, int64_t rows, int32_t width, int32_t activation, float act_param,
                       float* out, int64_t ld_out, void* stream);
int gnc_activation_backward_f32(const float* z, int64_t ld_z, const float* grad_act, int64_t ld_grad, int64_t rows,
                                int32_t width, int32_t activation, float act_param, float* grad_z, int64_t ld_out, void* stream);
int gnc_layer_norm_backward_f32(const float* y, int64_t ld_y, const float* gamma, const float* grad_out, int64_t ld_grad,
                                int64_t rows, int32_t width, float eps, float* grad_y, int64_t ld_gy, float* yhat,
                                int64_t ld_yhat, void* stream);

/* ---- K14: batch normalisation over table rows (added within ABI 20: new entry points only, nothing existing changes; two
 * host tests pin the version to 20) ---------------------------------------------------------
 * Replaces the `nn.BatchNorm1d(out_dim)` that models/MLP.py:29-35 appends for norm_type='BatchNorm1d' (the module runs at
 * models/MLP.py:47), its autograd, and - in eval mode - the op altogether.  z [rows, width] fp32, row stride ld >= width,
 * 1 <= width <= 256, any row count (64-bit row offsets).  Rows of 16-B pieces (width % 4 == 0, ld % 4 == 0, 16-B aligned
 * base) are read with vector loads, anything else with scalar loads by the same kernels.
 *
 * Training forward, three launches:
 *   gnc_bn_stats_f32     partial[b] = [ count (width) | mean (width) | M2 (width) ] of the b-th CONTIGUOUS range of rows,
 *                        gnc_bn_partials(rows, width) rows in all, every one fully written (no zero-initialised scratch).
 *                        Chunked two-pass + Chan merges: no sum-of-squares cancellation for columns with |mean| >> std.
 *   gnc_bn_finalize_f32  merges the partial rows in index order: mean[c], invstd[c] = 1 / sqrt(var + eps) (biased var), and,
 *                        where given (either may be NULL), in place
 *                          running_mean = (1 - momentum) running_mean + momentum mean
 *                          running_var  = (1 - momentum) running_var  + momentum var rows / (rows - 1)     (rows >= 2)
 *   gnc_bn_apply_f32     out = (z - mean) * invstd * gamma + beta (+ residual; NULL = none).  `out` may be `z`.
 * Backward, three launches:
 *   gnc_bn_backward_sums_f32  partial[b] = [ colsum(G) (width) | colsum(G * x_hat) (width) ], x_hat = (z - mean) * invstd
 *                             recomputed from z: the partial layout of gnc_colsum_pair_f32, gnc_bn_partials(rows, width) rows;
 *                             gnc_reduce_partials_f32(partial, parts, 2 * width, 2, width, sums, width, NULL) leaves
 *                             sums = [ d beta | d gamma ]
 *   gnc_bn_backward_dz_f32    grad_z = gamma * invstd * (G - d beta / rows - x_hat * d gamma / rows)
 *   (the gradient of the residual is grad_out itself)
 * Small tables (rows <= gnc_bn_small_max_rows(), the one-graph-per-step regime), ONE launch each way - a workgroup owns 4 columns
 * over all rows, so nothing is exchanged between workgroups and no scratch is needed:
 *   gnc_bn_forward_small_f32   statistics + running statistics + normalise (+ residual); also writes mean / invstd [width]
 *   gnc_bn_backward_small_f32  dbeta / dgamma [width] and grad_z (NULL: not wanted)
 * Eval mode:
 *   gnc_bn_fold_f32      weight_out[m, :] = s[m] weight[m, :], bias_out[m] = s[m] bias[m] + beta[m] - running_mean[m] s[m] with
 *                        s = gamma / sqrt(running_var + eps) (bias may be NULL = zeros): the last Linear of the MLP with the
 *                        normalisation folded in, so that one gnc_mlp_forward_f32 launch without a norm does everything
 *                        (residual and the edge-feature prologue included).  Call it on every forward: nothing is cached.
 * Fixed summation / merge order everywhere: bitwise reproducible, no float atomics.
 */
int gnc_bn_partials(int64_t rows, int32_t width);
int gnc_bn_stats_f32(const float* z, int64_t ld_z, int64_t rows, int32_t width, float* partial, int32_t num_partials, void* stream);
int gnc_bn_finalize_f32(const float* partial, int32_t num_partials, int64_t rows, int32_t width, float eps, float momentum,
                        float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
int gnc_bn_apply_f32(const float* z, int64_t ld_z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* residual, int64_t ld_res, int64_t rows, int32_t width, float* out, int64_t ld_out, void* stream);
int gnc_bn_backward_sums_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                             const float* invstd, int64_t rows, int32_t width, float* partial, int32_t num_partials, void* stream);
int gnc_bn_backward_dz_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                           const float* invstd, const float* gamma, const float* dbeta, const float* dgamma, int64_t rows,
                           int32_t width, float* grad_z, int64_t ld_gz, void* stream);
int gnc_bn_small_max_rows(void);
int gnc_bn_forward_small_f32(const float* z, int64_t ld_z, const float* gamma, const float* beta, const float* residual,
                             int64_t ld_res, int64_t rows, int32_t width, float eps, float momentum, float* out, int64_t ld_out,
                             float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
int gnc_bn_backward_small_f32(const float* grad_out, int64_t ld_grad, const float* z, int64_t ld_z, const float* mean,
                              const float* invstd, const float* gamma, int64_t rows, int32_t width, float* grad_z, int64_t ld_gz,
                              float* dbeta, float* dgamma, void* stream);
int gnc_bn_fold_f32(const float* weight, int64_t ld_w, const float* bias, const float* gamma, const float* beta,
                    const float* running_mean, const float* running_var, float eps, int32_t out_dim, int32_t in_dim,
                    float* weight_out, int64_t ld_wo, float* bias_out, void* stream);

/* ---- read-out classifier of ONE graph (ABI 18) -------------------------------------------------------------------
 * Replaces `LinearClassifier.forward` (models/GNN.py:312-325, called at :340) for the single-graph call of the reference's loops:
 * logits = fc3(relu(fc2(relu(fc1(y))))) over the flattened node outputs y [F]; weights as nn.Linear holds them.  One launch
 * forward (h1 [H1], h2 [H2]: the post-ReLU hidden vectors, kept for the backward; `ticket`: a device uint32 that is 0 before the
 * first launch and is left at 0 by every launch), one launch backward (all six parameter gradients, contiguous, and dy [F];
 * dy may be NULL).  H1, H2 <= 1024, C <= 64.  Fixed summation order (bitwise reproducible). */
int gnc_readout_forward_f32(const float* y, int64_t F, const float* w1, int64_t ld1, const float* b1, int32_t H1, const float* w2,
                            int64_t ld2, const float* b2, int32_t H2, const float* w3, int64_t ld3, const float* b3, int32_t C, float* h1,
                            float* h2, float* logits, uint32_t* ticket, void* stream);
int gnc_readout_backward_f32(const float* grad_logits, const float* y, int64_t F, const float* w1, int64_t ld1, int32_t H1, const float* w2,
                             int64_t ld2, int32_t H2, const float* w3, int64_t ld3, int32_t C, const float* h1, const float* h2, float* dw1,
                             float* db1, float* dw2, float* db2, float* dw3, float* db3, float* dy, void* stream);

/* ---- read-out classifier of G graphs: a block-diagonal batch (VERDICT row f4) --------------------------------------------------
 * logits [G, C] = fc3(relu(fc2(relu(fc1(feats))))) with the gather rule of `CombinedModel.forward_batched` applied where fc1's
 * operand is loaded: feature k * out_dim + j of graph g is y[start_g + k, j] for k < min(size_g, num_nodes) and 0 otherwise; no
 * [G, F] feature matrix is stored (F = num_nodes * out_dim).  `y` [n_total, out_dim] contiguous; `graph_ptr` DEVICE int64 [G + 1]
 * node offsets, or NULL: graph g owns rows [g num_nodes, (g + 1) num_nodes) and n_total == G num_nodes.  Offsets that point outside
 * y read as shorter or empty graphs, never outside the table.  Weights as nn.Linear holds them, read where they lie (row-major,
 * leading dimensions as in gnc_readout_forward_f32); biases may be NULL.
 *
 * Forward: fc1 on v_mfma_f32_16x16x4_f32, 16 graphs per workgroup, F split into `f_slices` slices whose partial [G, H1] tiles go
 * to `workspace` (`forward_workspace_floats` floats) and are summed in ascending slice order by the tail launch, which adds b1,
 * applies ReLU (NaN kept) and runs fc2 / fc3 from LDS.  h1 [G, H1], h2 [G, H2]: the post-ReLU activations, kept for the backward.
 * Backward: dw1 [H1, F] contiguous (columns no graph reaches: exact zeros), `small_grads` = [dW2 H2 x H1 | db2 H2 | dW3 C x H2 |
 * db3 C | db1 H1] contiguous, dy [n_total, out_dim] or NULL (every row written: rows a graph does not feed into fc1 get exact
 * zeros).  `workspace`: `backward_workspace_floats` floats, 16-B aligned.  Sums over graphs run over fixed chunks whose partials
 * are added in ascending order.  No atomics, no persistent counter, no memset: the workspaces belong to the call, results are
 * bitwise reproducible, every launch is a kernel node under stream capture.
 *
 * Served: H1 == 128, H2 <= 32, C <= 64, any F >= 1.  gnc_readout_batched_supported answers on the host (no device needed) from the
 * same decision the launchers read, and fills `plan` (may be NULL) with the split it chose; 1 = served.  The launchers return
 * GNC_ERR_UNSUPPORTED outside the set.  Added without an ABI bump: a library without these symbols fails the symbol lookup of
 * the binding. */
typedef struct gnc_readout_batched_plan {
  int64_t f_slices, f_slice_len;     /* forward: slices of F and their length (a multiple of 32)                        */
  int64_t tail_rows;                 /* graphs per workgroup of the tail launch                                         */
  int64_t small_parts;               /* backward: chunks of graphs behind the small gradients                           */
  int64_t dw1_parts, dw1_graph_range; /* backward: ranges of graphs behind dW1 and their length                         */
  int64_t dy_groups;                 /* backward: groups of graph tiles of the dy launch                                */
  int64_t forward_workspace_floats, backward_workspace_floats;
} gnc_readout_batched_plan_t;
int32_t gnc_readout_batched_supported(int64_t num_graphs, int64_t F, int32_t H1, int32_t H2, int32_t C,
                                      gnc_readout_batched_plan_t* plan);
int gnc_readout_batched_forward_f32(const float* y, const int64_t* graph_ptr, int64_t num_graphs, int64_t num_nodes, int32_t out_dim,
                                    int64_t n_total, const float* w1, int64_t ld1, const float* b1, int32_t H1, const float* w2,
                                    int64_t ld2, const float* b2, int32_t H2, const float* w3, int64_t ld3, const float* b3, int32_t C,
                                    float* h1, float* h2, float* logits, float* workspace, int64_t workspace_floats, void* stream);
int gnc_readout_batched_backward_f32(const float* grad_logits, const float* y, const int64_t* graph_ptr, int64_t num_graphs,
                                     int64_t num_nodes, int32_t out_dim, int64_t n_total, const float* w1, int64_t ld1, int32_t H1,
                                     const float* w2, int64_t ld2, int32_t H2, const float* w3, int64_t ld3, int32_t C, const float* h1,
                                     const float* h2, float* dw1, float* small_grads, float* dy, float* workspace,
                                     int64_t workspace_floats, void* stream);

/* ---- feed of a captured ragged mini-batch step ---------------------------------------------------
 * gnc_pad_graph_batch  ONE launch that writes every input buffer of a hipGraph captured over fixed capacities from a collated
 *                      block-diagonal batch: x [num_nodes, fx], pos [num_nodes, fp] (contiguous), edge_index [2, num_edges] int64
 *                      with ids already shifted (row stride ld_edge_index), and the HOST arrays graph_ptr / edge_ptr
 *                      [num_graphs + 1] and labels [num_graphs] (NULL with labels_buf NULL: none), which travel by value in the
 *                      kernel arguments - no host-to-device copy.  With M = node_capacity, C = edge_capacity and
 *                      D = max(1, ceil(C / 8)) dummy nodes:
 *                        x_buf [M + D, fx]: rows [0, N) = x, rows [N, M) = 0, rows [M, M + D) NOT written (the caller keeps them
 *                        zero); pos_buf likewise; ei_buf [2, C]: columns [0, E) = edge_index, column k >= E = (M + k % D,
 *                        M + k % D); graph_ptr_buf int64 [G + 1]; labels_buf int64 [G].
 *                      `flag` (device int32) is STICKY: 1 is stored when an end of an edge of graph g (edge_ptr says which) lies
 *                      outside [graph_ptr[g], graph_ptr[g + 1]); the kernel never clears it.  Ids are copied as given and not
 *                      dereferenced.  Sources need element alignment only (4 B floats, 8 B ids); 16-byte accesses are used
 *                      where the pointers allow.  Stream-ordered, no host synchronisation, a kernel node under stream capture.
 *                      Served: 1 <= num_graphs <= GNC_PAD_BATCH_MAX_GRAPHS (the 4 KB kernel-argument segment bounds it),
 *                      num_nodes <= M, num_edges <= C, M + D < 2^31; the query answers on the host without a device, the
 *                      launcher returns GNC_ERR_UNSUPPORTED outside the set before anything is launched.  Added without an ABI
 *                      bump: a library without these symbols fails the symbol lookup of the binding.
 */
#define GNC_PAD_BATCH_MAX_GRAPHS 64
int32_t gnc_pad_graph_batch_supported(int64_t num_graphs, int64_t num_nodes, int64_t num_edges, int64_t node_capacity,
                                      int64_t edge_capacity, int32_t fx, int32_t fp);
int gnc_pad_graph_batch(const float* x, int32_t fx, const float* pos, int32_t fp, const int64_t* edge_index,
                        int64_t ld_edge_index, int64_t num_nodes, int64_t num_edges, int64_t num_graphs,
                        const int64_t* graph_ptr, const int64_t* edge_ptr, const int64_t* labels, int64_t node_capacity,
                        int64_t edge_capacity, float* x_buf, float* pos_buf, int64_t* ei_buf, int64_t* graph_ptr_buf,
                        int64_t* labels_buf, int32_t* flag, void* stream);

/* ---- K17: global pooling read-out (csrc/pool_readout.hip) ----------------------------
 * Per graph g of a block-diagonal batch - rows [graph_ptr[g], graph_ptr[g + 1]) of `y` [rows, C] (float32, contiguous) - the column
 * sums, means (sum / float(n), a true fp32 division), maxima and the row index INTO y of each maximum.  `graph_ptr`: DEVICE int64
 * [num_graphs + 1], non-decreasing, never read on the host; rows outside [graph_ptr[0], graph_ptr[G]) (the slack and dummy rows
 * of a padded capture buffer) belong to no graph.  Offsets outside [0, rows] read as shorter or empty graphs, never outside y.
 * `modes`: GNC_POOL_* bits; exactly the outputs it names are non-NULL (argmax comes with max): psum / pmean / pmax [G, C] with row
 * pitch ld_out >= C (three column blocks of one [G, 3C] matrix, for instance), argmax int32 [G, C] contiguous.  Everything wanted
 * comes from ONE pass over y.
 *
 * Rules: an empty graph gives +0.0 everywhere and argmax -1; ties of the maximum go to the LOWEST row, -0.0 == +0.0; a NaN makes
 * its column's maximum NaN with argmax at the first NaN row and its sum NaN.  No atomics, no persistent counter, no memset: every
 * launch is a kernel node under stream capture.  The summation order depends on the graph's OWN rows and on C alone (chunks of
 * `chunk_rows` rows counted from the graph's first row, a fixed tree inside a chunk, ascending chunk order across): a graph pooled
 * alone and inside any batch gives the same bits, as do two runs.
 *
 * gnc_graph_pool_plan (host only, no device needed; 1 = served: rows < 2^31, 1 <= C <= 2^20, num_graphs >= 1) says which of two
 * regimes a launch takes, from rows / C / num_graphs alone - same bits either way: split == 0, one workgroup per (graph, column
 * tile); split == 1 (few large graphs), one workgroup per (chunk, column tile) writes partials into `workspace`
 * (`workspace_floats` floats, 4-B aligned, owned by the call) and a second launch folds them per graph in chunk order.
 *
 * Backward: dy [rows, C] contiguous, EVERY row written: dy[r, c] = dsum[g, c] + dmean[g, c] / float(n) + (argmax[g, c] == r ?
 * dmax[g, c] : 0) for a row r of a graph g with n rows (the terms whose pointer is NULL left out; a lone term is copied bit for
 * bit), exact zeros for rows of no graph.  dsum / dmean / dmax [G, C] share the row pitch ld_grad.  Added without an ABI bump: a
 * library without these symbols fails the symbol lookup of the binding. */
#define GNC_POOL_SUM 1
#define GNC_POOL_MEAN 2
#define GNC_POOL_MAX 4
typedef struct gnc_graph_pool_plan {
  int64_t chunk_rows;                              /* rows per chunk of the summation order                              */
  int64_t split;                                   /* 0: one workgroup per (graph, column tile); 1: per (chunk, tile) + merge */
  int64_t slots;                                   /* split: workspace slots = rows / chunk_rows + num_graphs            */
  int64_t vec, col_lanes, row_lanes, col_tiles;    /* the workgroup's tiling of [rows] x [columns], a function of C alone */
  int64_t workspace_floats;                        /* split: 3 * slots * C, otherwise 0                                  */
} gnc_graph_pool_plan_t;
int32_t gnc_graph_pool_plan(int64_t rows, int64_t C, int64_t num_graphs, gnc_graph_pool_plan_t* plan);
int gnc_graph_pool_forward_f32(const float* y, int64_t rows, int64_t C, const int64_t* graph_ptr, int64_t num_graphs, int32_t modes,
                               float* psum, float* pmean, float* pmax, int32_t* argmax, int64_t ld_out, float* workspace,
                               int64_t workspace_floats, void* stream);
int gnc_graph_pool_backward_f32(const float* dsum, const float* dmean, const float* dmax, int64_t ld_grad, const int32_t* argmax,
                                const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, int64_t C, float* dy, void* stream);

/* ---- K19: attention read-out (csrc/attention_pool.hip) ---------------------------------
 * Softmax-weighted global pooling with K17's conventions for `y` [rows, C], `graph_ptr` (DEVICE int64 [num_graphs + 1], never read
 * on the host, clamped into [0, rows]) and the rows of no graph, plus one score per row, `scores` [rows] float32.  For graph g with
 * rows [a, b):  m = max_v s_v,  e_v = expf(s_v - m) (the accurate expf),  Z = sum_v e_v,  out[g, c] = (sum_v e_v y[v, c]) / Z (an
 * IEEE division); `out` [G, C] with row pitch ld_out >= C.  An empty graph gives +0.0 and nothing is divided; rows of no graph are
 * never read.  `saved` [G, 2] floats receives (m, Z) per graph ((0, 0) for an empty one): the backward recomputes
 * alpha_v = expf(s_v - m) / Z from it, no [rows] array is kept.  Non-finite scores are outside the contract but stay inside their
 * graph: a NaN score makes every column of its own graph NaN, a NaN in y[v, c] column c of its graph, nothing else.
 *
 * Summation order: K17's, for Z and for the weighted column sums (chunks of `chunk_rows` rows from the graph's first row, the
 * fixed tree inside a chunk, ascending chunk order; e_v y[v, c] enters by one fmaf) - a graph pooled alone and inside any batch
 * gives the same bits, as do two runs.  The regime is gnc_graph_pool_plan's (rows, C, num_graphs alone; same bits either way):
 * split == 0, one launch of one workgroup per (graph, column tile); split == 1, three launches (the maxima, one workgroup per
 * (chunk, column tile) writing partials to `workspace`, the merge).  gnc_graph_attention_pool_workspace_floats: the floats the
 * call needs (0 outside the split regime: slots * (C + 1) in it; -1: sizes outside the served set, which is K17's - rows < 2^31,
 * 1 <= C <= 2^20, num_graphs >= 1; the launches then return GNC_ERR_UNSUPPORTED).  No atomics, no counters, no memset.
 *
 * Backward, ONE streaming launch over the rows: dy[v, :] = alpha_v dout[g, :] and ds[v] = alpha_v sum_c dout[g, c] (y[v, c] -
 * out[g, c]) (the softmax Jacobian with sum_u alpha_u (dout_g . y_u) = dout_g . out_g folded in; the dot over C in a fixed lane
 * order), exact +0.0 for rows of no graph.  `dout` [G, C] with row pitch ld_dout, `out` the forward's with pitch ld_out; dy
 * [rows, C] contiguous, ds [rows]; either may be NULL and is then skipped (y and out are only read for ds).
 * gnc_graph_attention_weights_f32 writes alpha [rows] (+0.0 for rows of no graph) from `scores` and `saved`.  Added without an ABI
 * bump: a library without these symbols fails the symbol lookup of the binding. */
int64_t gnc_graph_attention_pool_workspace_floats(int64_t rows, int64_t C, int64_t num_graphs);
int gnc_graph_attention_pool_forward_f32(const float* y, const float* scores, int64_t rows, int64_t C, const int64_t* graph_ptr,
                                         int64_t num_graphs, float* out, int64_t ld_out, float* saved, float* workspace,
                                         int64_t workspace_floats, void* stream);
int gnc_graph_attention_pool_backward_f32(const float* dout, int64_t ld_dout, const float* y, const float* scores, const float* out,
                                          int64_t ld_out, const float* saved, const int64_t* graph_ptr, int64_t num_graphs,
                                          int64_t rows, int64_t C, float* dy, float* ds, void* stream);
int gnc_graph_attention_weights_f32(const float* scores, const float* saved, const int64_t* graph_ptr, int64_t num_graphs,
                                    int64_t rows, float* alpha, void* stream);

/* ---- K20: top-K node pooling between the GN blocks (csrc/topk_pool.hip) ----------------
 * Graph g of a block-diagonal batch owns rows [a, b) of `graph_ptr` (DEVICE int64 [num_graphs + 1], clamped as K17's), n = b - a,
 * and keeps k_g = min(n, max(1, ceil(ratio n))) rows (product and ceiling in double; 0 for n = 0; 0 < ratio <= 1): the first k_g
 * of the total order "larger score first, -0.0 == +0.0, NaN below -inf, equal scores by lower row".  Kept rows keep their relative
 * order: new id = kept rows in front.  The result is a pure function of the scores' fp32 bits: the same alone, inside any batch
 * and twice.  No global atomics, no tickets, no memset: every output element is written by exactly one thread.
 *
 * gnc_topk_pool_select_f32: `scores` [rows] -> new_id int32 [rows] (-1: dropped; rows of no graph are dropped), kept int32 [N']
 * (old ids, ascending; allocate `rows`), new_graph_ptr int64 [num_graphs + 1], counts[0] = N' (counts: DEVICE int64 [2]).
 *
 * gnc_topk_pool_filter_edges: over the destination-sorted edge list src_sorted / dst_sorted int32 [E] and rowptr int32 [rows + 1]:
 * an edge survives when both endpoints are kept (an endpoint outside [0, rows) drops it and is never an index); survivors keep
 * their order, so dst_out stays sorted.  src_out / dst_out / kept_edges (old sorted positions, ascending) int32 [E'] (allocate E),
 * edge_new_id int32 [E] (-1: dropped), rowptr_out int32 [N' + 1] (allocate rows + 1): rowptr_out[v'] = kept edges in front of
 * rowptr[v], rowptr_out[N'] = E'; counts[1] = E' (counts[0] is read: run the select first, on the same stream).  `workspace`:
 * gnc_topk_pool_edge_workspace_ints(E) int32 (-1: E outside [0, 2^31)).
 *
 * Rows: out[i, :] = x[kept[i], :] * tanhf(scores[kept[i]]) for i < n_out (`scores` NULL: no gate, the bits of x); backward over
 * the rows_in input rows with j = new_id[r]: dx[r, :] = tanhf(s_r) dout[j, :], ds[r] = (1 - tanhf(s_r)^2) sum_c dout[j, c] x[r, c]
 * (the dot in a fixed lane order), exact +0.0 for a dropped row; every row of dx / ds is written once.  dx or ds may be NULL; ds
 * needs scores and x.  Leading dimensions >= C; 16-byte accesses when C % 4 == 0 and every table's rows are 16-byte aligned.
 * n_out is a HOST value: the caller reads counts back once per pooling layer.  Empty problems return GNC_OK.  Added without an
 * ABI bump: a library without these symbols fails the symbol lookup of the binding. */
int gnc_topk_pool_select_f32(const float* scores, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, double ratio,
                             int32_t* new_id, int32_t* kept, int64_t* new_graph_ptr, int64_t* counts, void* stream);
int64_t gnc_topk_pool_edge_workspace_ints(int64_t num_edges);
int gnc_topk_pool_filter_edges(const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* rowptr, int64_t num_edges,
                               int64_t rows, const int32_t* new_id, const int32_t* kept, int64_t* counts, int32_t* src_out,
                               int32_t* dst_out, int32_t* kept_edges, int32_t* edge_new_id, int32_t* rowptr_out, int32_t* workspace,
                               int64_t workspace_ints, void* stream);
int gnc_topk_pool_rows_forward_f32(const float* x, int64_t ld_x, int64_t rows_in, int64_t C, const int32_t* kept, int64_t n_out,
                                   const float* scores, float* out, int64_t ld_out, void* stream);
int gnc_topk_pool_rows_backward_f32(const float* dout, int64_t ld_dout, int64_t n_out, const float* x, int64_t ld_x, const float* scores,
                                    const int32_t* new_id, int64_t rows_in, int64_t C, float* dx, int64_t ld_dx, float* ds,
                                    void* stream);

/* The capacity-padded forms: the same arguments and the same launches, but every output is written over its
 * whole ALLOCATED length, so that a caller never reads counts back (a hipGraph capture can record the layer).  With N' / E' the
 * device counts, S_R = rows - N' and S_E = E - E':
 *   gnc_topk_pool_select_padded_f32    as the select, and kept[N', rows) = -1;
 *   gnc_topk_pool_filter_edges_padded  as the filter (run behind the padded select), and kept_edges[E', E) = -1; the edge at E' + t
 *     (0 <= t < S_E) is a self-loop of slack row N' + floor(t S_R / S_E) in src_out and dst_out (still destination-sorted, at most
 *     ceil(S_E / S_R) loops per slack row); rowptr_out[N' + u] = E' + ceil(u S_E / S_R) for 0 <= u <= S_R, so rowptr_out[rows] = E.
 *     S_R == 0 with S_E > 0 (only an edge with an endpoint outside [0, rows) can be dropped when every row is kept; the source
 *     topology's flags are set then): the slack loops go to row rows - 1 and rowptr_out[rows] = E.  rows == 0: nothing is launched.
 * The row launches then take n_out = rows (nodes) / E (edges): an id of -1 gives an exact +0.0 row, and the backward ignores
 * gradient rows that no new_id names.  Added without an ABI bump. */
int gnc_topk_pool_select_padded_f32(const float* scores, const int64_t* graph_ptr, int64_t num_graphs, int64_t rows, double ratio,
                                    int32_t* new_id, int32_t* kept, int64_t* new_graph_ptr, int64_t* counts, void* stream);
int gnc_topk_pool_filter_edges_padded(const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* rowptr, int64_t num_edges,
                                      int64_t rows, const int32_t* new_id, const int32_t* kept, int64_t* counts, int32_t* src_out,
                                      int32_t* dst_out, int32_t* kept_edges, int32_t* edge_new_id, int32_t* rowptr_out,
                                      int32_t* workspace, int64_t workspace_ints, void* stream);

/* ---- K24: k-nearest-neighbour edges inside every graph (csrc/knn_graph.hip) ------------
 * Node v scans every candidate u of its OWN graph (u == v only when loop != 0).  d(v, u) = sum_c (f_v[c] - f_u[c])^2 in fp32,
 * c ascending, from +0.0, subtract / multiply / add each rounded once (no fused multiply-add).  Candidates are ordered by the
 * 64-bit key (bits of d) << 32 | local index of u: smaller distance first, equal distances by the smaller node; a NaN distance
 * takes the distance field 0xffffffff and sets GNC_KNN_NAN_DISTANCE.  Edge slot v k + j holds the j-th smallest key of v: the
 * sender u in edge_index[0], the receiver v in edge_index[1], and in `dist` (may be NULL) the key's distance field as fp32.  A
 * graph with fewer candidates than k sets GNC_KNN_FEW_CANDIDATES; its unfillable slots hold -1 / -1 / +inf.  A pure function of
 * the features' bits: the same for a graph alone, inside any batch and twice.
 *
 *   gnc_knn_graph_f32         graph g owns rows [graph_ptr[g], graph_ptr[g+1]) (DEVICE int64 [num_graphs + 1], ascending, clamped
 *                             into [0, num_nodes]); ids are global; edge_index int64 [2, ld_edges], ld_edges >= k num_nodes; dist
 *                             fp32 [k num_nodes].  Rows of no graph are not written.
 *   gnc_knn_graph_padded_f32  the layout of gnc_rag_build_batched: feat [B, node_capacity, ld_feat], n_b = counts[b counts_stride]
 *                             read on the device (clamped into [0, node_capacity]); edge_index int64 [B, 2, k node_capacity] with
 *                             ids local to the image, dist fp32 [B, k node_capacity]; slots behind k n_b hold -1 / -1 / +inf, rows
 *                             behind n_b are never read.
 *
 * `status` (DEVICE int32 [1]) is zeroed by the call (a memset node ahead of the one kernel) and OR-ed into with an integer atomic,
 * the only atomic.  Stream-ordered, no host synchronisation, capturable; one launch sized from host values alone
 * (num_nodes / 64 + num_graphs, or B ceil(node_capacity / 64) workgroups).  Supported: 1 <= k <= 16, 1 <= dim <= 16,
 * ld_feat >= dim; GNC_ERR_UNSUPPORTED otherwise, decided before the first HIP call.  gnc_knn_graph_constants reports the query
 * rows of a workgroup and the unroll of its candidate loop (the sizes at which the kernel changes path).  Added without an
 * ABI bump: a library without these symbols fails the symbol lookup of the binding. */
enum { GNC_KNN_FEW_CANDIDATES = 1, GNC_KNN_NAN_DISTANCE = 2 };
int gnc_knn_graph_f32(const float* feat, int64_t ld_feat, int32_t dim, const int64_t* graph_ptr, int64_t num_graphs,
                      int64_t num_nodes, int32_t k, int32_t loop, int64_t* edge_index, int64_t ld_edges, float* dist,
                      int32_t* status, void* stream);
int gnc_knn_graph_padded_f32(const float* feat, int64_t ld_feat, int32_t dim, const int32_t* counts, int64_t counts_stride,
                             int32_t B, int32_t node_capacity, int32_t k, int32_t loop, int64_t* edge_index, float* dist,
                             int32_t* status, void* stream);
void gnc_knn_graph_constants(int32_t* query_block, int32_t* candidate_unroll);

/* ---- K18: mean / max neighbourhood aggregation (csrc/segment_reduce.hip) --------------
 * The node model's aggregation with another reducer than K1's sum, over the same destination-sorted CSR and with K1's argument
 * conventions: out[v, :] reduces src[row(k), :] over the sorted positions k in [rowptr[v], rowptr[v+1]), row(k) = perm[k] or k
 * itself when `perm` is NULL.  No atomics; rows are folded in ascending k (the sort is stable: original edge order); every out
 * row is written exactly once; two runs, and a graph alone or inside a block-diagonal batch, give the same bits.
 *   GNC_SEGMENT_MEAN: the running sum exactly as gnc_scatter_sum_csr_f32 forms it (from +0.0, ascending k), then sum / (float)deg,
 *                     a true fp32 division.  A destination without rows gives +0.0.  `argmax` must be NULL.
 *   GNC_SEGMENT_MAX:  the fold rule of K17: the larger value wins, a NaN beats everything (argmax at the first NaN), a tie goes to
 *                     the lowest sorted position, -0.0 == +0.0.  A destination without rows gives +0.0 and argmax -1.
 *                     `argmax`: NULL (inference: no extra store) or int32 [num_nodes, feat_dim] contiguous, the row of `src`
 *                     that won each column.
 * Backward, one pass over the num_rows rows of grad_src [num_rows, ld_src] (row r of grad_src belongs to row r of the forward's
 * src; dst_of_row[r] is its destination): MEAN writes grad_out[dst, :] / (float)deg(dst) (needs rowptr), MAX writes
 * grad_out[dst, c] where argmax[dst, c] == r and exact +0.0 elsewhere (needs argmax).  No [E, D] intermediate.
 * gnc_rows_div_degree_f32: in place, table[v, :] /= (float)deg(v) with the MEAN kernel's division; rows of degree 0 are left
 * alone.  Applied to a table of K1 sums (or of the fused aggregation epilogue) it gives the MEAN kernel's bits; it is linear, so
 * applied to the gradient it is its own backward.
 * All three: int status, no allocation, no synchronisation, kernel nodes under stream capture.  Added without an ABI bump: a
 * library without these symbols fails the symbol lookup of the binding. */
#define GNC_SEGMENT_MEAN 1
#define GNC_SEGMENT_MAX 2
int gnc_segment_reduce_csr_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* perm, int64_t num_nodes,
                               int64_t num_edges, int32_t feat_dim, int32_t mode, float* out, int64_t ld_out, int32_t* argmax,
                               void* stream);
int gnc_segment_reduce_backward_f32(const float* grad_out, int64_t ld_grad, const int32_t* dst_of_row, const int32_t* rowptr,
                                    const int32_t* argmax, int64_t num_nodes, int64_t num_rows, int32_t feat_dim, int32_t mode,
                                    float* grad_src, int64_t ld_src, void* stream);
int gnc_rows_div_degree_f32(float* table, int64_t ld, const int32_t* rowptr, int64_t num_nodes, int32_t feat_dim, void* stream);

/* ---- K21: attention neighbourhood aggregation (csrc/segment_softmax.hip) --------------
 * A softmax-weighted sum of every destination's incoming rows over K18's destination-sorted CSR, with K18's argument conventions:
 * row(k) = perm[k], or k itself when `perm` is NULL, indexes BOTH `src` [num_edges, ld_src] and `scores` [num_edges].
 *   m_v = max_k s_k (fmaxf from -inf: a NaN does not enter it);  e_k = expf(s_k - m_v);  Z_v = sum_k e_k;
 *   out[v, c] = (sum_k e_k x_k[c]) / Z_v, each product entering by one fmaf, both sums from +0.0 in ascending k, a true fp32
 *   division;  saved[v] = (m_v, Z_v), float [num_nodes, 2] contiguous.  A destination without rows gives +0.0 and saved (0, 0).
 * With all scores of a destination equal the output row has the bits of GNC_SEGMENT_MEAN.  A NaN score makes its own destination's
 * row (and Z) NaN and touches no other; a -inf score among finite ones adds nothing.  No atomics; two runs, a graph alone or
 * inside a block-diagonal batch, and sorted rows or rows behind `perm` give the same bits.
 * Backward, one pass over the num_rows rows (row r of grad_src and entry r of grad_scores belong to row r of the forward's src and
 * scores; dst_of_row[r] = d is its destination), alpha_r = expf(s_r - m_d) / Z_d recomputed from `saved`:
 *   grad_src[r, :] = alpha_r grad_out[d, :];   grad_scores[r] = alpha_r sum_c grad_out[d, c] (src[r, c] - out[d, c]).
 * gnc_segment_softmax_weights_f32 writes alpha [num_rows] alone.
 * All three: int status, no allocation, no synchronisation, no host read-back, kernel nodes under stream capture.  Added without an
 * ABI bump: a library without these symbols fails the symbol lookup of the binding. */
int gnc_segment_softmax_csr_f32(const float* src, int64_t ld_src, const float* scores, const int32_t* rowptr, const int32_t* perm,
                                int64_t num_nodes, int64_t num_edges, int32_t feat_dim, float* out, int64_t ld_out, float* saved,
                                void* stream);
int gnc_segment_softmax_backward_f32(const float* grad_out, int64_t ld_grad, const float* src, int64_t ld_src, const float* scores,
                                     const float* out, int64_t ld_out, const float* saved, const int32_t* dst_of_row,
                                     int64_t num_nodes, int64_t num_rows, int32_t feat_dim, float* grad_src, int64_t ld_gsrc,
                                     float* grad_scores, void* stream);
int gnc_segment_softmax_weights_f32(const float* scores, const float* saved, const int32_t* dst_of_row, int64_t num_rows, float* alpha,
                                    void* stream);

/* ---- graph construction on the device ---------------------------
 * Inputs: an already resized uint8 RGB image [H, W, C] in HBM.  Outputs: the tensors
 * utils/dataloader.py:49-51 builds (x, pos float32; edge_index int64 [2, E] row-major), in the
 * reference's node and edge order.
 *
 * gnc_grid_edges_i64   utils/image_to_graph/image_to_graph_optimized.py:7-39 (one-directional 4-neighbour
 *                      grid, optional two diagonal families); E = gnc_grid_num_edges().
 * gnc_pixel_nodes_f32  optimized.py:73-79: x = raw pixel values, pos = (row, col).
 * gnc_patch_nodes_f32  image_to_graph_patch.py:30-47: mean colour and integer centre per patch.
 * gnc_rag_build        image_to_graph_superpixel.py:36-71 after SLIC: `labels` [H, W] int32 in [0, H*W);
 *                      x [<=H*W, 3] mean of img/255 per label, pos = centroid (y, x), labels compacted in
 *                      ascending order (np.unique); edge_index rows have leading dimension ld_edges >=
 *                      4*H*W; counts[0] = segments, counts[1] = directed edges, counts[2] = 1 if a label
 *                      was out of range.
 */
int64_t gnc_grid_num_edges(int32_t H, int32_t W, int32_t diagonals);
int gnc_grid_edges_i64(int32_t H, int32_t W, int32_t diagonals, int64_t* edge_index, void* stream);
int gnc_pixel_nodes_f32(const uint8_t* img, int32_t H, int32_t W, int32_t C, float* x, float* pos, void* stream);
int gnc_patch_nodes_f32(const uint8_t* img, int32_t H, int32_t W, int32_t C, int32_t patch, float* x, float* pos,
                        void* stream);
size_t gnc_rag_workspace_bytes(int32_t H, int32_t W);
int gnc_rag_build(const int32_t* labels, const uint8_t* img, int32_t H, int32_t W, float* x, float* pos,
                  int64_t* edge_index, int64_t ld_edges, int32_t* counts, void* workspace, size_t workspace_bytes,
                  void* stream);

/* gnc_rag_build_batched  gnc_rag_build for B label images of one size in ONE launch, at fixed capacities and without
 *                      a host read: `labels` [B, H, W] int32, `img` [B, H, W, 3] uint8 -> x [B, node_capacity, 3],
 *                      pos [B, node_capacity, 2], edge_index [B, 2, edge_capacity], counts [B, 4] = (segments, directed
 *                      edges, 1 if a label was outside [0, H*W), 1 if the graph does not fit the capacities).  Per image
 *                      the first `segments` rows and `edges` columns equal gnc_rag_build's bit for bit; rows behind them
 *                      are 0, edge slots behind them -1.  An image whose overflow flag is set still reports its true
 *                      sizes (edges = -1 where it has more than 512 segments: the adjacency is not formed then) and its
 *                      slices hold padding only.  Supported: H*W <= 65536, node_capacity <= 512, edge_capacity <= 4096;
 *                      gnc_rag_batched_workspace_bytes returns 0 outside that set.  Integer atomics only
 *                      (deterministic), stream-ordered, no host synchronisation, safe under stream capture.  Added
 *                      without an ABI bump: a library without these symbols fails the symbol lookup of the binding.
 */
size_t gnc_rag_batched_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t node_capacity, int32_t edge_capacity);
int gnc_rag_build_batched(const int32_t* labels, const uint8_t* img, int32_t B, int32_t H, int32_t W,
                          int32_t node_capacity, int32_t edge_capacity, float* x, float* pos, int64_t* edge_index,
                          int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K26: region descriptors for superpixel nodes (csrc/region_descriptor.hip) ----
 * gnc_region_descriptors_rgb_u8  `labels` [B, H, W] int32 in [0, H*W) (gaps allowed; regions are numbered as gnc_rag_build
 *                      numbers them), `img` [B, H, W, 3] uint8 -> out [B, node_capacity, GNC_REGION_DESCRIPTOR_DIM] float32
 *                      (16-byte aligned) and counts [B, 3] = (regions, 1 if a label was outside [0, H*W), 1 if there are
 *                      more regions than node_capacity), in ONE launch.  Columns of a region with n pixels, from exact
 *                      integer sums, every expression evaluated in double and cast to float:
 *                        0-2   mean colour (S_c / 255) / n          = the x of gnc_rag_build, bit for bit
 *                        3-5   colour std  sqrt(n Q_c - S_c^2) / (255 n)
 *                        6     area share  n / (H W)
 *                        7, 8  bounding-box extent  (ymax - ymin + 1) / H, (xmax - xmin + 1) / W
 *                        9, 10 spatial spread  sqrt(n Syy - Sy^2) / (n H), sqrt(n Sxx - Sx^2) / (n W)
 *                        11    box fill  n / ((ymax - ymin + 1)(xmax - xmin + 1))
 *                        12    boundary share: pixels with a 4-neighbour of another label / n
 *                        13-15 texture: mean |v_c(p) - v_c(q)| / 255 over the horizontally and vertically adjacent pixel
 *                              pairs inside the region (0 without such a pair)
 *                      Rows behind the region count are zeros; a flagged image's slice is all zeros.  Supported:
 *                      H*W <= 65536, node_capacity <= 512, B <= 2^20; gnc_region_descriptors_workspace_bytes returns 0
 *                      outside that set.  Integer atomics only (deterministic), stream-ordered, no host synchronisation,
 *                      safe under stream capture.  Added without an ABI bump.
 */
#define GNC_REGION_DESCRIPTOR_DIM 16
size_t gnc_region_descriptors_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t node_capacity);
int gnc_region_descriptors_rgb_u8(const int32_t* labels, const uint8_t* img, int32_t B, int32_t H, int32_t W,
                                  int32_t node_capacity, float* out, int32_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- SLIC superpixels on the device (ABI 20; image_to_graph_superpixel.py:31) ------------------
 * gnc_slic_rgb_u8      scikit-image 0.18.3 `slic(img_as_float(img), n_segments, compactness, max_iter,
 *                      enforce_connectivity, min_size_factor, max_size_factor, start_label)` with sigma = 0, no
 *                      mask, unit spacing, slic_zero off and Lab conversion, for B images `img` [B, H, W, 3] uint8
 *                      at once.  `labels` [B, H, W] int32; counts[b] = labels handed out (connectivity on:
 *                      new labels of the connectivity pass; off: number of grid centres).  Workspace of
 *                      gnc_slic_workspace_bytes(B, H, W, n_segments) bytes (0 = shape not supported).
 *                      GNC_ERR_UNSUPPORTED for H or W > 4096, n_segments < 1, compactness <= 0, max_iter outside
 *                      1..1000, start_label other than 0 or 1, negative size factors.  Stream-ordered, no host
 *                      synchronisation.
 */
size_t gnc_slic_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_segments);
int gnc_slic_rgb_u8(const uint8_t* img, int32_t B, int32_t H, int32_t W, int32_t n_segments, double compactness,
                    int32_t max_iter, int32_t enforce_connectivity, double min_size_factor, double max_size_factor,
                    int32_t start_label, int32_t* labels, int32_t* counts, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- batched RGB resize on the device (the `Image.resize((R, R))` of every image_to_graph builder) --
 * gnc_resize_rgb_u8    Pillow's `Image.fromarray(img).resize((out_w, out_h), filter)` byte for byte for B uint8 RGB images
 *                      of any sizes at once; filter = PIL.Image.Resampling value: BILINEAR 2, BICUBIC 3 (Pillow's
 *                      default), BOX 4 (anything else: GNC_ERR_UNSUPPORTED).  `table` NULL: `src` is a dense
 *                      [B, in_h, in_w, 3] batch.  Otherwise `table` is DEVICE int64 [B, 3] = (byte offset of image b in
 *                      `src`, h_b, w_b) with 1 <= h_b <= in_h and 1 <= w_b <= in_w (an entry outside that is skipped).
 *                      `out` [B, out_h, out_w, 3] uint8.  Workspace of gnc_resize_workspace_bytes(B, in_h, in_w, out_h,
 *                      out_w, filter) bytes (0 = not supported: B or a side outside 1..65535, unknown filter).
 *                      Stream-ordered, no host synchronisation, safe under stream capture.  Added without an ABI bump:
 *                      a library without these symbols fails the symbol lookup of the binding.
 */
size_t gnc_resize_workspace_bytes(int32_t B, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t filter);
int gnc_resize_rgb_u8(const uint8_t* src, const int64_t* table, int32_t B, int32_t in_h, int32_t in_w, int32_t out_h,
                      int32_t out_w, int32_t filter, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K25: train-time image augmentation, pinned to Pillow (csrc/augment.hip) ---------------------
 * gnc_crop_resize_rgb_u8   `Image.fromarray(img_b).crop(box_b).resize((out_w, out_h), filter)`, then FLIP_LEFT_RIGHT where the
 *                      image's flag is set, byte for byte.  The arguments of gnc_resize_rgb_u8 and `boxes`: DEVICE int64 [B, 5] =
 *                      (left, top, right, bottom, flip) with 0 <= left < right <= w_b and 0 <= top < bottom <= h_b; a row outside
 *                      that is skipped (its output left as it was), never read out of bounds.  Crop, then resize: filter windows
 *                      clamp at the box (this is not `Image.resize(box=...)`, which reads outside the box).  The same three
 *                      launches as the resize; the flip is part of the last store.  Workspace of
 *                      gnc_crop_resize_workspace_bytes(B, in_h, in_w, out_h, out_w, filter) bytes, in_h / in_w being the largest
 *                      IMAGE sides (0 = not supported).  Stream-ordered, no host synchronisation, safe under stream capture.
 * gnc_color_jitter_rgb_u8  Pillow's ImageEnhance.Brightness / .Contrast / .Color chains, byte for byte, IN PLACE on a dense uint8
 *                      [B, H, W, 3] batch.  `order` DEVICE int32 [B, 3]: the operations of image b in the order they run
 *                      (0 brightness, 1 contrast, 2 color; any other value, or a repeated one, is no operation); `factor` DEVICE
 *                      float32 [B, 3] indexed by operation.  A factor of 1 is the identity and costs nothing.  One launch, one
 *                      workgroup per image, no workspace, no atomics; images of up to gnc_color_jitter_resident_pixels() pixels
 *                      wait in the LDS across the contrast's reduction, larger ones are read twice.  Sides <= 65535.
 *                      Stream-ordered, a kernel node under stream capture.
 * Added without an ABI bump: a library without these symbols fails the symbol lookup of the binding.
 */
size_t gnc_crop_resize_workspace_bytes(int32_t B, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t filter);
int gnc_crop_resize_rgb_u8(const uint8_t* src, const int64_t* table, const int64_t* boxes, int32_t B, int32_t in_h, int32_t in_w,
                           int32_t out_h, int32_t out_w, int32_t filter, uint8_t* out, void* workspace, size_t workspace_bytes,
                           void* stream);
int64_t gnc_color_jitter_resident_pixels(void);
int gnc_color_jitter_rgb_u8(uint8_t* img, int32_t B, int32_t H, int32_t W, const int32_t* order, const float* factor,
                            void* stream);

/* gnc_u8_hwc_to_f32_chw  torchvision's ToTensor for B uint8 images [B, H, W, C] on the device: out [B, C, H, W] float32 with
 *                      out[b, c, y, x] = float(img[b, y, x, c]) / 255 (a correctly rounded division: bit for bit what
 *                      `t.permute(2, 0, 1).float().div(255)` gives).  B, C <= 65535.  Stream-ordered, a kernel node under stream
 *                      capture.  Added without an ABI bump: a library without this symbol fails the symbol lookup of the binding.
 */
int gnc_u8_hwc_to_f32_chw(const uint8_t* img, int32_t B, int32_t H, int32_t W, int32_t C, float* out, void* stream);

/* ---- K16: split-K first Linear of an MLP over a wide input (csrc/wide_linear.hip) ----------------
 * a0 = act(x W^T + bias) for x [rows, K] (row pitch ld_x >= K, any alignment: rows that are not 16-B aligned are read with dword
 * loads), W [H, K] as nn.Linear stores it (row pitch ld_w >= K, any alignment), bias [H] or NULL, activation one of GNC_ACT_*.
 * Forward, two launches: partial products of [16 rows] x [all H outputs] x [one slice of K] on fp32 MFMA into `workspace`
 * ([k_slices, rows, H padded to 16]), then a tail launch that sums the slices in ascending order, adds the bias, stores the
 * pre-activation into z0 (when not NULL: the backward of an activation other than ReLU reads it) and the activation into a0.
 * Backward, from grad_a0 [rows, H]: dz0 = grad_a0 * act'(.), where `az` is a0 for GNC_ACT_RELU and z0 for every other activation;
 * dw [H, K] contiguous = dz0^T x, db [H] = column sums of dz0.  Row ranges (dw_parts of dw_row_range rows) are summed in ascending
 * order through `workspace` (backward_workspace_floats floats, 16-B aligned; may be NULL when that is 0).  The gradient of x is not
 * formed.  No atomics, no persistent counter, no memset: results are bitwise reproducible and every launch is a kernel node under
 * stream capture.
 *
 * Served: 1 <= rows <= 512 (the batch sizes timed against the row-tiled kernels; larger batches stay with those), 1024 <= K <= 2^26,
 * 1 <= H <= 256.  gnc_wide_linear_supported answers on the host (no device needed)
 * for a fused-MLP description, from the same decision the launchers read: 1 when the description is ONE row-ordered matmul segment
 * (no index, no additive segment, no residual, no aggregation or edge-feature prologue, no save_act) in front of at least two
 * Linears and its rows, in_dim[0], out_dim[0] are in the set; `plan` (may be NULL) receives the split.  The caller then runs the
 * first Linear here and the remaining Linears + norm as an ordinary description over a0.  gnc_wide_linear_workspace_floats: floats
 * of the forward (backward != 0: backward) workspace, -1 outside the set.  The launchers return GNC_ERR_UNSUPPORTED outside the
 * set before anything is launched.  Added without an ABI bump: a library without these symbols fails the symbol lookup of the
 * binding. */
typedef struct gnc_wide_linear_plan {
  int64_t k_slices, k_slice_len;    /* forward: slices of K and their length (a multiple of 32); the last one may be shorter */
  int64_t dw_parts, dw_row_range;   /* backward: ranges of rows behind dw / db and their length (a multiple of 16)          */
  int64_t forward_workspace_floats, backward_workspace_floats;
} gnc_wide_linear_plan_t;
int32_t gnc_wide_linear_supported(const gnc_mlp_desc_t* desc, gnc_wide_linear_plan_t* plan);
int64_t gnc_wide_linear_workspace_floats(int64_t rows, int64_t K, int32_t H, int32_t backward);
int gnc_wide_linear_forward_f32(const float* x, int64_t ld_x, int64_t rows, int64_t K, const float* w, int64_t ld_w,
                                const float* bias, int32_t H, int32_t activation, float act_param, float* a0, int64_t ld_a,
                                float* z0, int64_t ld_z, float* workspace, int64_t workspace_floats, void* stream);
int gnc_wide_linear_backward_f32(const float* grad_a0, int64_t ld_grad, const float* az, int64_t ld_az, const float* x,
                                 int64_t ld_x, int64_t rows, int64_t K, int32_t H, int32_t activation, float act_param, float* dw,
                                 float* db, float* workspace, int64_t workspace_floats, void* stream);

/* ---- fused Adam over flat buffers -------------------------------
 * Replaces `optimizer.step()` of utils/train_model.py:42 for `optim.Adam(model.parameters(), lr=1e-3)` (:9):
 * every parameter is a view of `param` [n], every gradient a view of `grad` [n]; one launch updates all of them
 * with torch.optim.Adam's arithmetic (amsgrad off).  `step` is a DEVICE int64 holding the number of updates made
 * so far (the call advances it first; bias corrections are derived from it on the device in double precision), so
 * the call sequence is the same on every step and can be replayed from a hipGraph.  `scratch2` is 2 floats of
 * device scratch.  All four buffers 16-B aligned.
 * gnc_adam_step_hp64_f32 takes lr and the betas as doubles, as Python holds them: the bias corrections and the weights
 * 1 - beta of the element update are then torch.optim.Adam's, each rounded to fp32 once (a beta rounded to fp32 first
 * moves 1 - beta by up to 1.3e-5 and 1 - beta^t by up to 3.7e-6 of itself).  gnc_adam_step_f32 widens its floats, which
 * is Adam with the betas' fp32 values throughout.
 */
int gnc_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t* step, float* scratch2,
                      void* stream);
int gnc_adam_step_hp64_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                           double beta1, double beta2, float eps, float weight_decay, int64_t* step, float* scratch2,
                           void* stream);

/* ---- controlled optimizer step: clipping, AdamW / SGD, learning-rate schedules (K22, csrc/optimizer_ctl.hip) ----
 * Everything that steers an update lives on the device, so ONE captured step replays a schedule, clips and skips:
 *   gnc_grad_sumsq_f32   sum of g * g over grad [n] into `partials` (GNC_GRAD_NORM_BLOCKS doubles), one double per workgroup
 *                        of a FIXED grid (GNC_GRAD_NORM_PASS elements per grid pass): no atomics, the order - and so the bits -
 *                        depend on n alone.  An fp32 x fp32 product is exact in double.
 *   gnc_optimizer_ctl_step_f32   [the sum pass, when ctl->clip or ctl->check_nonfinite] + a one-workgroup control tick + one
 *                        element launch.  The tick sums the partials in fixed order and derives, in double and rounded to fp32
 *                        once, into `scalars` [GNC_OPT_SCALARS]: [0] step_size (Adam / AdamW: lr(t) / (1 - beta1^t); SGD: lr(t)),
 *                        [1] sqrt(1 - beta2^t), [2] decay = 1 - lr(t) * weight_decay (AdamW, else 1), [3] clip_coef =
 *                        min(1, max_grad_norm / (norm + 1e-6)) (1 without clipping), [4] lr(t), [5] the gradient norm BEFORE
 *                        clipping (NaN when the sum pass did not run); t = *step + 1 is stored back to `step`.
 *                        lr(t): base lr * (t / warmup_steps) for t <= warmup_steps, then constant, cosine to min_lr at
 *                        total_steps (held afterwards) or lr * gamma^((t - warmup_steps) / every).
 *                        A non-finite sum (with clip or check_nonfinite) SKIPS the step: `step`, the parameters and the state
 *                        stay bit-unchanged, skipped[0] (a running count) is advanced and skipped[1] (this call's flag) set;
 *                        [5] still reports the norm.  torch.nn.utils.clip_grad_norm_ would scale every gradient by NaN instead.
 *                        The element launch reads g' = fl(clip_coef * g); `grad` itself is never written.
 * state1 / state2: exp_avg / exp_avg_sq (Adam, AdamW), or the momentum buffer (zero-initialised; may be null when momentum
 * == 0) / null (SGD).  param, grad and the state buffers 16-B aligned; `step` int64 [1], `skipped` int64 [2]. */
enum { GNC_OPT_ADAM = 0, GNC_OPT_ADAMW = 1, GNC_OPT_SGD = 2 };
enum { GNC_LR_CONSTANT = 0, GNC_LR_COSINE = 1, GNC_LR_STEP = 2 };
#define GNC_GRAD_NORM_BLOCKS 256
#define GNC_GRAD_NORM_PASS (GNC_GRAD_NORM_BLOCKS * 256 * 4)
#define GNC_OPT_SCALARS 8

typedef struct gnc_opt_ctl_t {
  int32_t rule;            /* GNC_OPT_*                                                              */
  int32_t schedule;        /* GNC_LR_*                                                               */
  int32_t nesterov;        /* SGD: d = g + momentum * buf                                            */
  int32_t clip;            /* scale the gradient to max_grad_norm (implies check_nonfinite)          */
  int32_t check_nonfinite; /* skip the step when the gradient holds a NaN or an inf                  */
  int32_t reserved;
  int64_t warmup_steps, total_steps, every; /* in optimizer steps                                    */
  double lr, min_lr, gamma, max_grad_norm;
  double beta1, beta2, eps, weight_decay, momentum;
} gnc_opt_ctl_t;

int32_t gnc_sizeof_opt_ctl(void);
int64_t gnc_grad_norm_pass(void);
int32_t gnc_grad_norm_blocks(void);
int gnc_grad_sumsq_f32(const float* grad, int64_t n, double* partials, void* stream);
int gnc_optimizer_ctl_step_f32(float* param, const float* grad, float* state1, float* state2, int64_t n, const gnc_opt_ctl_t* ctl,
                               int64_t* step, float* scalars, int64_t* skipped, double* partials, void* stream);

/* ---- classification loss head: weighted / smoothed cross-entropy, binary cross-entropy, training metrics (K23, csrc/class_loss.hip) ----
 * gnc_class_loss_f32: logits fp32 [G, C] (row stride ld_logits), labels int64 [G], class_weight fp32 [C] or null (w = 1).
 *   GNC_LOSS_CE   torch.nn.CrossEntropyLoss(weight=w, label_smoothing=s):  lp = log_softmax(z_i), W = sum_c w_c,
 *                 row_i = -(1 - s) w[y_i] lp[y_i] - (s / C) sum_c w_c lp[c];  den = sum_i w[y_i] (MEAN) or 1 (SUM)
 *   GNC_LOSS_BCE  binary_cross_entropy_with_logits(z, t, pos_weight=pw) on ONE logit per row (C == 1, class_weight null), labels
 *                 0 or 1, t_i = y_i (1 - s) + s / 2:  row_i = pw t_i softplus(-z_i) + (1 - t_i) softplus(z_i);  den = rows (MEAN)
 *   loss [1] = scale * sum_i row_i / den;  dlogits [G, C] (row stride ld_dlogits; null: scoring only) = d loss / d logits.
 *   loss_sum (double [1], or null) += the returned fp32 loss.  confusion (int64 [K, K], or null; K = C, BCE: 2; rows = the label)
 *   += the counts of (label, predicted class): argmax_c z_ic with the lowest index on ties (BCE: z > 0), inside [0, K) whatever the
 *   logits hold.  status (int32 [1]) |= 1 when a label lies outside [0, K): that row adds nothing to loss, den, the counts, and its
 *   dlogits row is zeros; nothing is indexed with the label.  den == 0: loss and dlogits are 0.
 * Rows in fp32 (accurate exp / log), sums over rows in double in an order that (G, C) alone decide; no floating-point atomics.
 * With GNC_LOSS_SUM a row's dlogits have the same bits alone and inside any batch.
 * G <= GNC_CLASS_LOSS_ONE_LAUNCH_ROWS: ONE kernel launch, `workspace` may be null.  Above: rows pass, one-workgroup tick, gradient
 * pass (gnc_class_loss_launches tells), over `workspace` (GNC_CLASS_LOSS_WORKSPACE_DOUBLES doubles, overwritten).
 * Nothing is allocated or synchronised. */
enum { GNC_LOSS_CE = 0, GNC_LOSS_BCE = 1 };
enum { GNC_LOSS_MEAN = 0, GNC_LOSS_SUM = 1 };
#define GNC_CLASS_LOSS_ONE_LAUNCH_ROWS 64 /* == GNC_PAD_BATCH_MAX_GRAPHS: every captured mini-batch */
#define GNC_CLASS_LOSS_BLOCKS 256
#define GNC_CLASS_LOSS_WORKSPACE_DOUBLES (2 * GNC_CLASS_LOSS_BLOCKS + 1)

int32_t gnc_class_loss_workspace_doubles(void);
int32_t gnc_class_loss_launches(int64_t G, int32_t with_gradient);
int gnc_class_loss_f32(const float* logits, int64_t ld_logits, const int64_t* labels, const float* class_weight, int64_t G, int64_t C,
                       int32_t kind, double label_smoothing, double pos_weight, int32_t reduction, double scale, float* loss,
                       float* dlogits, int64_t ld_dlogits, double* loss_sum, int64_t* confusion, int32_t* status, double* workspace,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNC_HIP_H */
