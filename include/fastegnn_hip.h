/*
 * fastegnn_hip.h -- C ABI of libfastegnn_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for ONE path of GLAD-RUC/FastEGNN: the forward and backward of the
 * FastEGNN model (reference: models/FastEGNN.py:192-276 + autograd, utils/train.py:169).
 * The reference has no FFI for this path (it is a Python nn.Module calling ATen); the entry
 * points below are what a binding for it needs: plain pointers + sizes + a hipStream_t, the
 * caller allocates every buffer, no torch types, no global mutable state, re-entrant per
 * stream.  Each function returns 0 on success or a negative FASTEGNN_E_* code;
 * fastegnn_last_error() gives the message of the calling thread's last failure.
 *
 * All device arrays are fp32 row-major unless noted; indices are int32.
 * H (hidden_nf) is fixed to 64 in this build.
 *
 * One E_GCL_vel layer (models/FastEGNN.py:192-223) is evaluated as five stages; on one GPU
 * fastegnn_layer_forward/backward chain them, a sharded caller runs the stages itself and
 * exchanges the marked buffers between them (DESIGN.md "Multi-GPU").
 *
 *   forward                              backward (reverse order)
 *   S1 node_pre   h -> P, QX, A, heads    B1 node_pre_bwd
 *   S2 graph_pre  x,Z,Hv -> Bc            B3 graph_pre_bwd
 *   S3 edge       P,QX,CSR -> aggm,aggx   B2 edge_bwd (+ col-keyed reduce)
 *   S4 virt       ... -> h',x',pools      B4 virt_bwd
 *   S5 graph_post pools -> Z',Hv'         B5 graph_post_bwd
 */
#ifndef FASTEGNN_HIP_H
#define FASTEGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASTEGNN_H 64
#define FASTEGNN_QX_LD 68 /* source-table row: Q[64] | x[3] | pad */

enum {
  FASTEGNN_OK = 0,
  FASTEGNN_E_INVALID = -1, /* bad argument (null pointer, unsupported size) */
  FASTEGNN_E_LAUNCH = -2,  /* HIP launch / runtime failure */
  FASTEGNN_E_NODEVICE = -3 /* no gfx950 device visible */
};

/* constructor flags of the reference model (models/FastEGNN.py:227-228, :11-12) */
enum {
  FASTEGNN_F_ATTENTION = 1,
  FASTEGNN_F_NORMALIZE = 2,
  FASTEGNN_F_TANH = 4,
  FASTEGNN_F_RESIDUAL = 8,
  FASTEGNN_F_GRAVITY = 16,
  FASTEGNN_F_COORDS_SUM = 32, /* coords_agg='sum' (default 'mean') */
  /* EGNN baseline layer (models/basic.py:285-320) on the same kernels: C = 0 (no virtual nodes),
   * edge_mlp.0 columns ordered [radial | h_row | h_col | edge_attr] (:313), coordinate head with bias,
   * aggregated coordinate message clamped to +-100 (:310), no residual on h, velocity head optional */
  FASTEGNN_F_EGNN = 64,
  /* FastRF reduced layer (models/FastRF.py:155-186) on the same kernels: node_mlp / node_mlp_virtual are
   * absent (h and the virtual features pass through unchanged, their parameter slots are null) and the
   * velocity scale is coord_mlp_vel(||vel||) with coord_mlp_vel.0.weight of shape [H,1] (:76-80,:139) */
  FASTEGNN_F_RF = 128,
  /* bf16 operand mode (BASELINE configs[2]; the reference has no reduced-precision mode): BOTH operands of every
   * 64-wide contraction -- the [64,64] weights and the 64-column blocks of edge_mlp.0 / edge_mlp_virtual.0 / node_mlp.0 /
   * node_mlp_virtual.0, in the forward, the input-gradient and the weight-gradient products -- are rounded to bf16
   * (round to nearest even) and multiplied on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  Coordinates, radial /
   * vr / Gram terms and their weight columns, edge_attr / node_attr columns, the [1,64] heads, attention gates, biases,
   * activations, segment sums and pools stay fp32.  Mirror: oracle/factored.py with Config.bf16. */
  FASTEGNN_F_BF16 = 256,
  /* EGNN(norm=True) (models/basic.py:271-272): the 1x1 Gram feature of the message MLP is F.normalize'd -- r^2 / max(r^2, 1e-12),
   * i.e. 1 for every edge of non-zero length (gradient 0) and r^2 * 1e12 below (gradient 1e12).  With FASTEGNN_F_EGNN only. */
  FASTEGNN_F_EGNN_NORM = 512,
  /* Backward only.  By default the col-side adjoint of the edge stage -- d loss / d (Q | x)[col], the transpose of the
   * forward gather -- is scattered into g_QX_src with fp32 atomics (one coalesced 272-byte row per edge): g_QXe, the CSC
   * index of the graph (cscptr / csc_eid may then be NULL, also in fastegnn_build_csr) and fastegnn_edge_col_reduce's
   * kernel are not used, and the sums depend on the order the atomics land in (rounding-level run-to-run differences,
   * like torch's scatter_add_ on a GPU).  With this flag the rows are stored per edge in g_QXe [E,68] and summed in CSC
   * order by fastegnn_edge_col_reduce: that sum is then order-independent (the rest of the backward keeps its
   * rounding-level run-to-run differences: pools and ticket-ordered in-workgroup sums); 0.26 ms per step slower at cfg4 in
   * fp32, faster than the atomics with bf16 operands; 272 bytes of scratch per edge. */
  FASTEGNN_F_DETERMINISTIC = 1024,
  /* Backward, atomic mode only: fastegnn_edge_backward does NOT zero g_QX_src before it scatters into it -- an earlier
   * launch of the same layer over OTHER rows has already done so.  The sharded caller runs a rank's boundary rows (rows
   * with an edge from a ghost column) and its interior rows as two launches, so that the ghost rows' gradients travel
   * while the interior rows are still being computed (bits 11..14 hold the activation kind, below). */
  FASTEGNN_F_GQX_ACCUM = 32768,
  /* Forward: wpack already holds this layer's weight images (fastegnn_pack_weights_all packed every layer of the model in
   * one launch): fastegnn_layer_forward / fastegnn_pack_weights skip the per-layer pack launch. */
  FASTEGNN_F_WPACK_READY = 65536
};
/* Activation of every MLP (the reference's act_fn, models/FastEGNN.py:227): bits 11..14 of the flags hold one of the
 * FASTEGNN_ACT_* kinds, fastegnn_layer_t.act_param its parameter.  libfastegnn_hip.so is compiled for SiLU and rejects
 * any other kind (FASTEGNN_E_ARG); libfastegnn_hip_act.so (same sources, -DFE_ACT_GENERIC) evaluates all of them. */
#define FASTEGNN_F_ACT_SHIFT 11
#define FASTEGNN_F_ACT_MASK 15
enum {
  FASTEGNN_ACT_NONE = -1,        /* fastegnn_wide_linear*: no fused activation */
  FASTEGNN_ACT_SILU = 0,
  FASTEGNN_ACT_RELU = 1,
  FASTEGNN_ACT_LEAKY_RELU = 2,   /* act_param = negative_slope */
  FASTEGNN_ACT_TANH = 3,
  FASTEGNN_ACT_SIGMOID = 4,
  FASTEGNN_ACT_ELU = 5,          /* act_param = alpha */
  FASTEGNN_ACT_GELU = 6,         /* exact (erf) form */
  FASTEGNN_ACT_SOFTPLUS = 7      /* act_param = beta; threshold 20 as torch.nn.Softplus */
};

/* Per-layer parameter slots: the reference state_dict tensors of gcl_<i>, untouched
 * ([out,in] row-major as torch stores them).  models/FastEGNN.py:28-99. */
enum {
  FASTEGNN_P_EDGE0_W = 0, /* edge_mlp.0.weight          [64, 128+1+ea] */
  FASTEGNN_P_EDGE0_B,     /* edge_mlp.0.bias            [64] */
  FASTEGNN_P_EDGE2_W,     /* edge_mlp.2.weight          [64,64] */
  FASTEGNN_P_EDGE2_B,
  FASTEGNN_P_VIRT0_W,     /* edge_mlp_virtual.0.weight  [64, 128+1+C] */
  FASTEGNN_P_VIRT0_B,
  FASTEGNN_P_VIRT2_W,     /* edge_mlp_virtual.2.weight  [64,64] */
  FASTEGNN_P_VIRT2_B,
  FASTEGNN_P_ATT_W,       /* att_mlp.0.weight           [1,64]   (null unless attention) */
  FASTEGNN_P_ATT_B,       /* att_mlp.0.bias             [1] */
  FASTEGNN_P_ATTV_W,      /* att_mlp_virtual.0.weight   [1,64] */
  FASTEGNN_P_ATTV_B,
  FASTEGNN_P_CR0_W,       /* coord_mlp_r.0.weight       [64,64] */
  FASTEGNN_P_CR0_B,
  FASTEGNN_P_CR2_W,       /* coord_mlp_r.2.weight       [1,64] (no bias) */
  FASTEGNN_P_CRV0_W,      /* coord_mlp_r_virtual.*      */
  FASTEGNN_P_CRV0_B,
  FASTEGNN_P_CRV2_W,
  FASTEGNN_P_CVV0_W,      /* coord_mlp_v_virtual.*      */
  FASTEGNN_P_CVV0_B,
  FASTEGNN_P_CVV2_W,
  FASTEGNN_P_VEL0_W,      /* coord_mlp_vel.0.weight     [64,64] */
  FASTEGNN_P_VEL0_B,
  FASTEGNN_P_VEL2_W,      /* coord_mlp_vel.2.weight     [1,64] */
  FASTEGNN_P_VEL2_B,      /* [1] */
  FASTEGNN_P_GRAV0_W,     /* gravity_mlp.*  (null unless gravity) */
  FASTEGNN_P_GRAV0_B,
  FASTEGNN_P_GRAV2_W,
  FASTEGNN_P_GRAV2_B,
  FASTEGNN_P_NODE0_W,     /* node_mlp.0.weight          [64, 128+64*C+na] */
  FASTEGNN_P_NODE0_B,
  FASTEGNN_P_NODE2_W,     /* node_mlp.2.weight          [64,64] */
  FASTEGNN_P_NODE2_B,
  FASTEGNN_P_NODEV0_W,    /* node_mlp_virtual.0.weight  [64,128] */
  FASTEGNN_P_NODEV0_B,
  FASTEGNN_P_NODEV2_W,    /* node_mlp_virtual.2.weight  [64,64] */
  FASTEGNN_P_NODEV2_B,
  FASTEGNN_P_CR2_B,       /* coord head bias [1] (EGNN baseline only: coord_net.mlp.2.bias) */
  FASTEGNN_P_COUNT
};

/* Sorted graph produced by fastegnn_build_csr (replaces the implicit scatter indices of
 * unsorted_segment_sum/mean, models/FastEGNN.py:279-294). */
typedef struct {
  int32_t n_rows;          /* aggregation targets owned by this rank (== N on one GPU) */
  int32_t n_src;           /* rows of the source table the col indices address */
  int32_t n_edges;
  int32_t n_chunks;        /* edge-balanced row chunks (work items of the edge kernels) */
  const int32_t *rowptr;   /* [n_rows+1] */
  const int32_t *erow;     /* [E] row of sorted edge */
  const int32_t *col;      /* [E] source-table index of sorted edge */
  const int32_t *perm;     /* [E] sorted edge k == input edge perm[k] */
  const int32_t *cscptr;   /* [n_src+1] */
  const int32_t *csc_eid;  /* [E] sorted-edge ids grouped by col */
  const int32_t *chunk_row;/* [n_chunks+1] first row of each chunk */
} fastegnn_graph_t;

/* Everything one layer call touches.  "in"/"out" are w.r.t. the forward; the backward reads
 * the saved buffers and the g_* inputs and writes the g_* outputs (accumulating into grads). */
typedef struct {
  /* sizes / flags */
  int32_t N, B, C, ea, na, flags;
  float gravity[3];
  float epsilon;           /* models/FastEGNN.py:21 */
  float act_param;         /* parameter of the activation kind in the flags (FASTEGNN_ACT_*); 0 for SiLU */
  fastegnn_graph_t graph;
  const int32_t *batch;    /* [N] graph id per node, ascending */
  const int32_t *gptr;     /* [B+1] node range of each graph */
  const float *ea_sorted;  /* [E,ea] edge_attr in sorted-edge order */
  const float *vel;        /* [N,3] */
  const float *node_attr;  /* [N,na] or null */

  const float *const *params; /* HOST array [FASTEGNN_P_COUNT] of device pointers */
  float *const *grads;        /* HOST array [FASTEGNN_P_COUNT] of device pointers (+=), backward only */
  float *wpack;               /* packed MFMA weight images, fastegnn_wpack_floats(C) floats */

  /* layer inputs (saved for backward by the caller) */
  const float *h;          /* [N,64] */
  const float *x;          /* [N,3] */
  const float *Z;          /* [B,3,C]   virtual coordinates (reference layout) */
  const float *HvT;        /* [B,C,64]  virtual features, channel-major */
  /* layer outputs.  h_out == NULL && HvT_out == NULL (FastEGNN wiring, i.e. neither FASTEGNN_F_RF nor FASTEGNN_F_EGNN): the node update of
   * this layer is not wanted -- node_model and node_model_virtual are not run (nothing reads h / Hv after the last layer of FastEGNN),
   * x_out and Z_out are what they are otherwise; npre and poolV are then not written and may be null too.  Exactly one of the two null
   * is FASTEGNN_E_INVALID (checked before any launch), as a null h_out is under the other two wirings. */
  float *h_out, *x_out, *Z_out, *HvT_out;

  /* stage products (saved for backward) */
  float *P;                /* [N,64]   S1 */
  float *QX;               /* [N,68]   S1: Q | x | pad.  (sharded: all-gathered into QX_src) */
  const float *QX_src;     /* [n_src,68] table the edge kernels gather from (== QX on one GPU) */
  float *A;                /* [N,64]   S1 */
  float *svel, *sgrav;     /* [N]      S1 */
  float *xsum;             /* [B,4]    S2: per-graph sum of x | node count (sharded: all-reduced) */
  float *Bc;               /* [B,C,64] S2 */
  float *aggm;             /* [N,64]   S3 */
  float *aggx;             /* [N,3]    S3 */
  float *npre;             /* [N,64]   S4: node_mlp pre-activation */
  float *poolV;            /* [B,C,64] S4 (sum over nodes; sharded: all-reduced) */
  float *poolX;            /* [B,3,C]  S4 (sum over nodes; sharded: all-reduced) */

  /* backward inputs: d loss / d layer outputs.  g_h_out == NULL && g_HvT_out == NULL (FastEGNN wiring): no gradient arrives for h / Hv, and
   * the forward of this layer ran without its node update (above) -- the adjoint of node_model / node_model_virtual is not run, grads[] of
   * node_mlp.* and node_mlp_virtual.* are left untouched, npre, poolV and g_poolV are not read and may be null; g_h, g_x, g_Z, g_HvT
   * and every other gradient are what a zero g_h_out / g_HvT_out gives.  Exactly one of the two null is FASTEGNN_E_INVALID. */
  const float *g_h_out, *g_x_out, *g_Z_out, *g_HvT_out;
  /* backward outputs: d loss / d layer inputs.
   * fastegnn_layer_backward only, FastEGNN wiring with the atomic scatter (no FASTEGNN_F_DETERMINISTIC / _RF / _EGNN: FASTEGNN_E_INVALID before
   * any launch there), as for g_vel / g_ea_sorted / g_node_attr below -- null means "not wanted":
   *   g_x == NULL  d loss / d x is not wanted (the first layer of a model whose positions need no gradient): the edge stage forms no
   *                coordinate adjoint (no g_xrow sums, no coordinate atomic), the virtual stage carries no g_x from channel to channel, the
   *                graph and node_pre stages write neither g_x nor g_xbar.  g_xrow and g_xbar must still be valid scratch; they are not touched.
   *   g_Z == NULL  d loss / d Z is not wanted: the graph stages write no g_Z; with g_x null as well the virtual stage does not form g_Zp.
   * Every other gradient is what it is with the pointers set.  The staged entry points require both, as before ("null buffer"). */
  float *g_h, *g_x, *g_Z, *g_HvT;
  float *g_vel;            /* [N,3] accumulated (+=), may be null */
  float *g_ea_sorted;      /* [E,ea] d loss / d edge_attr in sorted-edge order, accumulated (+=) over the layers; null: not wanted */
  float *g_node_attr;      /* [N,na] d loss / d node_attr, accumulated (+=) over the layers; null: not wanted */

  /* backward scratch (caller allocates; the shapes below, the wg_* sizes from fastegnn_wg_*_floats, the total from
   * fastegnn_backward_scratch_floats) */
  float *g_poolV, *g_poolX;   /* [B,C,64], [B,3,C] */
  float *g_Bc;                /* [B,C,64] (sharded: all-reduced before B3) */
  float *g_Zp;                /* [B,3,C]  partial from B4 (sharded: all-reduced) */
  float *g_xbar;              /* [B,3]    per-node share of d/d centroid */
  float *g_A, *g_P, *g_aggm;  /* [N,64] */
  float *g_aggx;              /* [N,3] */
  float *g_svel, *g_sgrav;    /* [N] */
  float *g_QXe;               /* [E,68]  per-edge d/d(Q|x) of the col side */
  float *g_QX_src;            /* [n_src,68] col-keyed sums (sharded: reduce-scattered).  fastegnn_layer_backward with g_QX == g_QX_src,
                               * n_src == N, the atomic scatter, no FASTEGNN_F_GQX_ACCUM and a base that is a multiple of 128 bytes uses the
                               * same N * 68 floats as a Q block [N,64] followed by an x block [N,4]: the 256-byte atomic row of an edge then
                               * lies in two 128-byte lines instead of three.  Scratch either way: nothing outside the call reads it. */
  float *g_QX;                /* [N,68]  this rank's slice of g_QX_src (== g_QX_src on one GPU) */
  float *g_xrow;              /* [N,3]   row-side d/dx of the edge stage */
  float *wg_edge;             /* [fastegnn_wg_edge_floats(E)] weight-gradient operands of the edge stage (none when the
                               * edge backward contracts them inside the workgroup: 4 floats then) */
  float *wg_virt;             /* [fastegnn_wg_virt_floats_for(N,C,flags)] weight-gradient operands of the virtual stage */
  float *wg_node;             /* [fastegnn_wg_node_floats(N,B,C)] node-level weight-gradient operands */
  float *wg_slab;             /* [fastegnn_wg_slab_floats()] partial 64x64 slabs of the weight-gradient GEMMs */
  /* Backward STAGE entry points only (fastegnn_layer_backward keeps its own): an open weight-gradient batch
   * (fastegnn_wgrad_batch_open) into which the stage queues its contraction jobs instead of contracting and reducing them
   * itself -- ONE contraction launch and ONE reduction launch per layer for a caller that drives the stages one by one
   * (the sharded path, which has collectives between them).  The operands a stage queues (its g_* outputs and its region
   * of wg_node) must stay untouched until fastegnn_wgrad_batch_close.  NULL: the stage finishes its own jobs. */
  void *wgrad_batch;
} fastegnn_layer_t;

/* ---- library ---- */
const char *fastegnn_last_error(void);
/* ABI revision: FASTEGNN_ABI_VERSION of the header the library was built from.  It changes whenever the layout of
 * fastegnn_layer_t / fastegnn_graph_t or the meaning of an argument changes (round 3 inserted act_param: 100 -> 101; round 4 appended wgrad_batch and added fastegnn_pack_weights_all / FASTEGNN_F_WPACK_READY: 103; the fastegnn_wide_* entry points: 104;
 * round 5: fastegnn_f16_operands / fastegnn_check_finite: 105; the fused activation arguments of fastegnn_wide_linear / _dx / _dw: 106;
 * round 6: fastegnn_host_words_alloc / _free, fastegnn_zero_if_flagged, fastegnn_check_finite writes 1 instead of OR-ing: 107;
 * fastegnn_adam_step_v2 with a step count per tensor: 108).
 * A purely ADDITIVE export -- a new function that leaves every descriptor and every existing argument as it was -- does not
 * bump the revision: a binding finds it by symbol, and an older library fails that lookup (fastegnn_grad_sqnorm,
 * fastegnn_adam_step_dev and their size queries were added at 108 this way).
 * A binding MUST compare it with the FASTEGNN_ABI_VERSION it was written against AND check fastegnn_sizeof_layer() /
 * fastegnn_sizeof_graph() against its own mirror of the descriptors before the first call (fastegnn_amd/_lib.py does). */
#define FASTEGNN_ABI_VERSION 108
int fastegnn_version(void);
/* floats of the packed weight-image buffer for C virtual channels */
size_t fastegnn_wpack_floats(int32_t C);
/* floats of the weight-gradient slab workspace (independent of the problem size) */
size_t fastegnn_wg_slab_floats(void);
size_t fastegnn_wg_edge_floats(int32_t E);
size_t fastegnn_wg_virt_floats(int32_t N, int32_t C);
size_t fastegnn_wg_node_floats(int32_t N, int32_t B, int32_t C);
/* wg_virt: three of the virtual stage's weight gradients are contracted inside the workgroup, so the workspace is ONE
 * [C][N+16][64] array plus constant-size part tiles and consumer scratch (~36 MB at C = 16; 4 floats at C = 0).  Until
 * round 4 the FastRF / EGNN wirings kept five arrays and the size depended on the flags; every wiring has the one form
 * now and the _for variant (kept for ABI stability) ignores `flags`. */
size_t fastegnn_wg_virt_floats_for(int32_t N, int32_t C, int32_t flags);
/* floats of all backward scratch arrays of fastegnn_layer_t together (g_poolV ... wg_slab), each array rounded up to
 * a multiple of 4 floats so that one allocation can be carved into 16-byte aligned pieces */
size_t fastegnn_backward_scratch_floats(int32_t N, int32_t E, int32_t n_src, int32_t B, int32_t C);
size_t fastegnn_backward_scratch_floats_for(int32_t N, int32_t E, int32_t n_src, int32_t B, int32_t C, int32_t flags);
/* A weight-gradient batch shared by the backward stage calls of ONE layer (fastegnn_layer_t.wgrad_batch).  open: L gives
 * wg_slab (the batch takes the lower half of the slab workspace, as fastegnn_layer_backward's does) and the operand mode;
 * the stages must run on `stream`.  close: contracts and reduces everything queued (two launches), then frees the handle --
 * also call it after a failed stage.  Host-side objects only: capturable. */
int fastegnn_wgrad_batch_open(const fastegnn_layer_t *L, void *stream, void **batch);
int fastegnn_wgrad_batch_close(void *batch);
/* struct sizes, so that a foreign-language binding can verify its mirror of the descriptors */
size_t fastegnn_sizeof_layer(void);
size_t fastegnn_sizeof_graph(void);

/* ---- graph preprocessing (COO int64, any order -> row-sorted CSR + col-keyed index) ----
 * edge_index: device int64 [2,E] as the reference passes it (models/FastEGNN.py:204).
 * Rows must lie in [row_begin, row_begin+n_rows) and are stored relative to row_begin; cols
 * address the source table [0,n_src).  All outputs caller-allocated:
 * rowptr[n_rows+1], erow/col/perm/csc_eid[E], cscptr[n_src+1], chunk_row[fastegnn_chunk_rows(E)]
 * (row boundaries nearest to every 32nd edge: the edge kernels give each wave a contiguous run of them);
 * tmp: fastegnn_csr_tmp_bytes(E, n_rows, n_src) bytes.  *n_chunks is a host int.
 * The index is the STABLE sort's (edges of a row keep the caller's order): built with rocPRIM radix sorts, or -- edge lists of
 * at most 600 000 edges with at most 64 edges per id on average -- by counting (count, scan, place, rank inside the id), which gives
 * the same arrays element for element; FASTEGNN_CSR_SORT=radix|count in the environment forces one form.
 * The edge stages address their tables with 32-bit offsets: n_rows * 68 and n_src * 68 must stay below 2^30
 * (15.7 M nodes) and E * 8 below 2^30 (134 M edges); fastegnn_edge_forward / _backward return
 * FASTEGNN_E_INVALID beyond that. */
size_t fastegnn_csr_tmp_bytes(int32_t E, int32_t n_rows, int32_t n_src);
size_t fastegnn_chunk_rows(int32_t E);
int32_t fastegnn_chunk_edges(void);   /* edges per row chunk: chunk k owns the rows whose first edge lies in [k*T, (k+1)*T) */
int fastegnn_build_csr(const int64_t *edge_index, int32_t E, int32_t row_begin, int32_t n_rows,
                       int32_t n_src, int32_t *rowptr, int32_t *erow, int32_t *col, int32_t *perm,
                       int32_t *cscptr, int32_t *csc_eid, int32_t *chunk_row, int32_t *n_chunks,
                       void *tmp, size_t tmp_bytes, void *stream);
/* out[k,:] = in[perm[k],:]   (edge_attr into sorted order) */
int fastegnn_permute_rows(const float *in, const int32_t *perm, int32_t E, int32_t width, float *out,
                          void *stream);
/* hidden_nf < 64: the kernels work on 64-wide tiles, a narrower model runs zero-padded (a zero row of a Linear gives a
 * zero pre-activation, SiLU(0) = 0, a zero column ignores its input: the padded model computes the reference's function,
 * models/FastEGNN.py:28-99 with hidden_nf = h).  One descriptor per parameter: `src` [rows, cols] row-major is copied into
 * `dst` [rows_dst, cols_dst] (zero elsewhere); the first `nblk` column blocks of blk[i] source columns each -- the
 * hidden-sized pieces of the reference's torch.cat inputs, FastEGNN.py:104,114,157,171 -- are widened to
 * blk[i] / h * 64 columns (zeros appended to the block), the remaining columns follow unchanged; `lead` source columns
 * in front of the first block are copied as they are (the radial column of the EGNN baseline's message MLP, basic.py:313).
 * reverse != 0 runs the
 * adjoint: src[r, c] = dst[r, map(c)] (the gradient of the narrow parameter is the matching slice of the padded one).
 * `desc` is a HOST array; at most 64 descriptors travel per launch (kernel arguments, capturable into a HIP graph). */
typedef struct {
  const float *src;        /* reverse: written */
  float *dst;              /* reverse: read */
  int32_t rows, cols;      /* of src */
  int32_t rows_dst, cols_dst;
  int32_t nblk;
  int32_t blk[3];
  int32_t lead;            /* unchanged columns in front of the blocks */
  int32_t reserved;
} fastegnn_pad_desc_t;
int fastegnn_pad_params(const fastegnn_pad_desc_t *desc, int32_t n, int32_t h, int32_t reverse, void *stream);
/* 1 when the library evaluates every FASTEGNN_ACT_* kind (libfastegnn_hip_act.so), 0 for the SiLU-only build */
int fastegnn_generic_activations(void);
/* 1 if the fp32-grade products of this build run on 2-part fp16 splits (operands must stay below 65 504 in magnitude: the default
 * library), 0 if on 3-part bf16 splits with fp32's exponent range (libfastegnn_hip_x3.so / _act_x3.so).  ABI revision 105. */
int fastegnn_f16_operands(void);
/* Range guard of the f16x2 build (the reference is plain fp32, models/FastEGNN.py:102-119: it has no such limit): *flag = 1 if any
 * of a[0..na) / b[0..nb) is not finite (a plain store of the constant: `flag` may be device memory OR a host-mapped word of
 * fastegnn_host_words_alloc, which the host then reads without any synchronisation).  One capturable launch on `stream`.
 * Either array may be NULL with its count 0.  ABI revision 105; store instead of atomic OR since 107. */
int fastegnn_check_finite(const float *a, int64_t na, const float *b, int64_t nb, int32_t *flag, void *stream);
/* n zero-initialised int32 words of pinned, host-MAPPED, coherent memory: kernels write them through the same address (the guard
 * launch above), the host polls them with plain loads -- no stream synchronisation, no copy, valid inside a captured HIP graph as
 * well.  The reference's only host synchronisation on this path is data_batch[-1].item() (models/FastEGNN.py:267), which the module
 * does not need; this keeps the range guard from adding one.  ABI revision 107. */
int fastegnn_host_words_alloc(int32_t n, int32_t **words);
int fastegnn_host_words_free(int32_t *words);
/* buf[0..n) = 0 if *flag != 0 (flag: device or host-mapped word).  The backward of a forward whose outputs left the f16x2 range
 * hands ZERO parameter gradients to the optimizer instead of NaNs (the host may not have seen the flag yet).  ABI revision 107. */
int fastegnn_zero_if_flagged(float *buf, int64_t n, const int32_t *flag, void *stream);
/* The channel-phased virtual backward hands work between the waves of a workgroup through LDS flags; since round 6 every wait on such a
 * flag is bounded (~0.3 s).  Returns how many waits have given up since the last reset -- 0 unless the hand-off protocol has a bug (the
 * launch then finished with wrong results instead of hanging the device); < 0: the query failed.  SYNCHRONISES the device: for tests and
 * post-mortems, not for the step.  ABI revision 107. */
int fastegnn_spin_timeouts(int reset);
/* Which specialised path did the layer calls take?  out[FASTEGNN_PATH_COUNT] receives the number of fastegnn_layer_forward /
 * fastegnn_layer_backward calls since the last reset that returned FASTEGNN_OK after taking
 *   FASTEGNN_PATH_NO_AGGM     forward, h_out == NULL && HvT_out == NULL: the edge stage did not build aggm (it feeds node_model alone; the
 *                             buffer itself stays non-null: it parks the per-block coordinate sums ahead of the edge stage)
 *   FASTEGNN_PATH_ZERO_GAGGM  backward, g_h_out == NULL && g_HvT_out == NULL: the zero rows of this layer's part of g_h were neither filled
 *                             nor read, and g_aggm was a plain fill (the staged entry points fill and read both as before)
 *   FASTEGNN_PATH_NO_GX       backward, g_x == NULL: no coordinate gradient of the layer inputs was formed (fastegnn_layer_t.g_x)
 *   FASTEGNN_PATH_SPLIT_GQX   backward: g_QX_src was used as a Q block [N,64] followed by an x block [N,4] (see g_QX_src)
 * reset != 0 clears the counts.  Host-side counters, no device work, not thread-safe: for tests.  FASTEGNN_KEEP_DEAD_EDGE_WORK=1 in the
 * environment (a DIAGNOSTIC, read per call) makes the layer calls run the unspecialised stages.  An additive export (revision 108). */
enum { FASTEGNN_PATH_NO_AGGM = 0, FASTEGNN_PATH_ZERO_GAGGM = 1, FASTEGNN_PATH_NO_GX = 2, FASTEGNN_PATH_SPLIT_GQX = 3, FASTEGNN_PATH_COUNT = 4 };
int fastegnn_path_counts(int64_t *out, int32_t reset);
/* batch int64 [N] (ascending) -> batch int32 [N], gptr int32 [B+1] */
int fastegnn_build_batch(const int64_t *batch64, int32_t N, int32_t B, int32_t *batch, int32_t *gptr,
                         void *stream);

/* ---- model prologue / epilogue (models/FastEGNN.py:267-271) ---- */
/* h = node_feat @ W^T + b   (embedding_in) */
int fastegnn_embed_forward(const float *node_feat, int32_t N, int32_t nf, const float *W, const float *b,
                           float *h, void *stream);
/* gW += g_h^T node_feat, gb += colsum g_h, g_node_feat = g_h W (nullable) */
int fastegnn_embed_backward(const float *node_feat, const float *g_h, int32_t N, int32_t nf, const float *W,
                            float *gW, float *gb, float *g_node_feat, void *stream);
/* HvT[b,c,:] = virtual_node_feat[0,:,c]  (the .repeat(B,1,1) of :268, channel-major) */
int fastegnn_virtual_init(const float *vnf, int32_t B, int32_t C, float *HvT, void *stream);
/* g_vnf[0,h,c] += sum_b g_HvT[b,c,h] */
int fastegnn_virtual_init_backward(const float *g_HvT, int32_t B, int32_t C, float *g_vnf, void *stream);

/* ---- one layer, staged ---- */
int fastegnn_pack_weights(const fastegnn_layer_t *L, void *stream);
/* The weight images of n layers of ONE model (same C, ea, na, flags; each descriptor needs params, wpack and the sizes) in one
 * launch: a layer's images are 34 + 2C small workgroups, and four launches of them cost four launch latencies in front of a step
 * that is otherwise 74 launches.  Set FASTEGNN_F_WPACK_READY in the flags of the layer calls that follow. */
int fastegnn_pack_weights_all(const fastegnn_layer_t *const *layers, int32_t n, void *stream);
int fastegnn_node_pre_forward(const fastegnn_layer_t *L, void *stream);   /* S1 */
int fastegnn_graph_xsum(const fastegnn_layer_t *L, void *stream);         /* S2a: local xsum */
int fastegnn_graph_pre_forward(const fastegnn_layer_t *L, void *stream);  /* S2b: xsum -> Bc */
int fastegnn_edge_forward(const fastegnn_layer_t *L, void *stream);       /* S3 */
int fastegnn_virt_forward(const fastegnn_layer_t *L, void *stream);       /* S4 (zeroes + fills pools) */
int fastegnn_graph_post_forward(const fastegnn_layer_t *L, void *stream); /* S5 */

int fastegnn_graph_post_backward(const fastegnn_layer_t *L, void *stream); /* B5 */
int fastegnn_virt_backward(const fastegnn_layer_t *L, void *stream);       /* B4 */
int fastegnn_graph_pre_backward(const fastegnn_layer_t *L, void *stream);  /* B3 */
int fastegnn_edge_backward(const fastegnn_layer_t *L, void *stream);       /* B2a: per-edge */
int fastegnn_edge_col_reduce(const fastegnn_layer_t *L, void *stream);     /* B2b: g_QXe -> g_QX_src */
int fastegnn_node_pre_backward(const fastegnn_layer_t *L, void *stream);   /* B1 */

/* ---- one layer, whole (single GPU): pack + S1..S5 / B5..B1 on the stream ---- */
int fastegnn_layer_forward(const fastegnn_layer_t *L, void *stream);
int fastegnn_layer_backward(const fastegnn_layer_t *L, void *stream);

/* ---- training-step closure (the harness code that brackets the hot path, utils/train.py) ----
 * out[e,:] = [edge_attr[e,:k] | ||loc[row_e]-loc[col_e]||]                      (utils/train.py:41-43) */
int fastegnn_augment_edge_attr(const int64_t *edge_index, const float *loc, const float *edge_attr, int32_t E,
                               int32_t k, float *out, void *stream);
/* loss2[0] = MSE(loc_pred,loc_t) + weight*(l_vv - l_rv), loss2[1] = MSE      (utils/train.py:104-165, kernel :17-20);
 * sample_nodes int32 [B,S]: absolute ids of the sampled real nodes of each graph; writes d loss / d loc_pred into
 * g_loc [N,3] and d loss / d virtual_node_loc into g_vloc [B,3,C]. */
int fastegnn_loss_mse_mmd(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                          int32_t N, int32_t B, int32_t C, int32_t S, float sigma, float weight, float *loss2,
                          float *g_loc, float *g_vloc, void *stream);
/* torch.optim.Adam step (no amsgrad, L2 weight decay; main_nbody.py:137) over n_tensors tensors given as HOST arrays
 * of device pointers; a tensor whose grads[i] is null is skipped entirely, as torch.optim.Adam skips parameters whose
 * .grad is None (no weight decay, no moment update).  steps (HOST, n_tensors): each tensor's own step count including
 * this step, from 1 -- torch.optim.Adam's state['step'], which advances only on steps where the parameter has a .grad
 * and sets the tensor's bias correction; not read for a tensor whose grads[i] is null.  The hyper-parameters are double,
 * as torch.optim.Adam holds them: 1 - beta and the bias corrections are formed before any rounding to fp32.
 * ABI revision 108. */
int fastegnn_adam_step_v2(float *const *params, const float *const *grads, float *const *exp_avg,
                          float *const *exp_avg_sq, const int64_t *numel, int32_t n_tensors, const int32_t *steps,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream);
/* the same with one step count for every tensor (the form of revisions up to 107) */
int fastegnn_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                       const int64_t *numel, int32_t n_tensors, int32_t step, float lr, float beta1, float beta2,
                       float eps, float weight_decay, void *stream);

/* ---- capturable optimizer step: every per-step quantity lives in DEVICE memory, so that a captured HIP graph that holds
 * these launches can be replayed for every training iteration (torch.optim.Adam(capturable=True)).
 * ADDITIVE exports: they change no descriptor and no existing argument, so FASTEGNN_ABI_VERSION stays 108 -- a binding
 * finds them by symbol (fastegnn_amd/_lib.py lists them in EXPORTED; a library without them fails that lookup loudly).
 *
 * Sum of squares over all present gradients (HOST arrays of device pointers as for fastegnn_adam_step_v2; a null entry
 * contributes nothing), written as ONE double to *out (device).  Two stages, no atomics: every workgroup writes its
 * fp64 partial into `ws` (fastegnn_grad_sqnorm_partials(numel, n) doubles: the slot of a workgroup is fixed by the tensor
 * sizes alone, not by which gradients are present), then one workgroup sums the slots in a fixed order -- run-to-run
 * identical, capturable.  Every product is exact (fp32 x fp32 in fp64); a non-finite element gives a non-finite *out. */
size_t fastegnn_grad_sqnorm_partials(const int64_t *numel, int32_t n_tensors);
int fastegnn_grad_sqnorm(const float *const *grads, const int64_t *numel, int32_t n_tensors, double *ws,
                         size_t ws_doubles, double *out, void *stream);
/* fastegnn_adam_step_v2 with its per-step state on the device:
 *   steps_dev  int32 [n_tensors], DEVICE: each tensor's step count, read AND advanced by this call;
 *   hyper_dev  double [6], DEVICE: lr, beta1, beta2, eps, weight_decay, max_grad_norm (<= 0: no clipping);
 *   sqnorm_dev double, DEVICE, may be null: fastegnn_grad_sqnorm's result (required when max_grad_norm > 0 is wanted:
 *              without it no clipping happens);
 *   skip_word  int32, device OR host-mapped (fastegnn_host_words_alloc), may be null: the range guard's word;
 *   scratch    fastegnn_adam_dev_scratch_bytes(n_tensors) bytes, DEVICE, 16-byte aligned: written and read by this call only.
 * If *skip_word != 0, or *sqnorm_dev is not finite, NOTHING moves: parameters, moments and steps_dev stay bitwise as they
 * were (a loss scaler's skipped step).  Otherwise every tensor with a non-null gradient advances its count by one and takes
 * torch.optim.Adam's update with the bias correction of its OWN new count, formed in fp64 on the device; with clipping
 * each gradient is multiplied by min(1, max_grad_norm / (sqrt(*sqnorm_dev) + 1e-6)) as it is read
 * (torch.nn.utils.clip_grad_norm_'s coefficient; the gradient buffers are not rewritten).  A tensor with a null
 * gradient is untouched.  One single-workgroup prologue launch takes the decision and advances the counts; the element
 * launches that follow on the stream read only what it wrote into `scratch`. */
size_t fastegnn_adam_dev_scratch_bytes(int32_t n_tensors);
int fastegnn_adam_step_dev(float *const *params, const float *const *grads, float *const *exp_avg,
                           float *const *exp_avg_sq, const int64_t *numel, int32_t n_tensors, int32_t *steps_dev,
                           const double *hyper_dev, const double *sqnorm_dev, const int32_t *skip_word, void *scratch,
                           size_t scratch_bytes, void *stream);

/* ---- the device-side MMD sample (utils/train.py:118-142: one torch.randperm(n_i)[:num_sample] per graph and step) ----
 * ADDITIVE exports, found by symbol like the ones above: FASTEGNN_ABI_VERSION stays 108.
 *
 *   rng  DEVICE uint64[2] = {seed, draw counter};  ptr  DEVICE int64 [B+1], ascending (the collate's data['ptr']).
 * For graph b with n = ptr[b+1] - ptr[b] (< 2^31):  sample_count[b] = min(S, n);
 *   n <= S : sample_nodes[b, j] = ptr[b] + j            for j < n
 *   n >  S : sample_nodes[b, j] = ptr[b] + perm_b(j)    for j < S, perm_b a keyed bijection of [0, n)
 * and the entries j >= sample_count[b] of row b are written as -1.  sample_nodes int32 [B,S], sample_count int32 [B].
 * advance != 0: a stream-ordered one-thread launch BEHIND the draw adds 1 to rng[1]; the draw itself only reads rng, so every
 * workgroup of one draw sees the same counter.  B == 0 launches no draw; S == 0 writes only the counts (all 0); both still
 * advance.  FASTEGNN_E_INVALID before any launch for: null rng / ptr, null sample_nodes with B * S > 0, null sample_count
 * with B > 0, B < 0, S < 0, S > 4096 (the loss's ceiling).  Capturable: replays of a captured draw read the counter the previous
 * replay left, so every replay draws a fresh sample.
 *
 * perm_b, in unsigned integer arithmetic only (uint64 sums and products wrap; a test mirrors it bit for bit):
 *   mix64(x):  z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *              return z ^ (z >> 31)                                                   (splitmix64's output function)
 *   mix32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16   (uint32, products wrap)
 *   k    = max(2, ceil(log2 n)) rounded up to even;  h = k / 2;  mask = 2^h - 1      (the domain 2^k is below 4 n for n >= 2)
 *   g    = mix64(mix64(mix64(seed) ^ counter) ^ (uint64) b)
 *   key_r = mix64(g + r),  r = 0 .. 7
 *   E(x): for r = 0 .. 7:  L = x >> h;  R = x & mask;  F = (mix32((uint32) R ^ (uint32) key_r) ^ (uint32)(key_r >> 32)) & mask;
 *                          x = (R << h) | (L ^ F)                                     (a balanced Feistel network: a bijection of [0, 2^k))
 *   perm_b(j):  x = E(j);  while x >= n: x = E(x);  return x                          (cycle walking)
 * E is a bijection, so perm_b is one of [0, n) and the S entries of a row are distinct.  The walk from a start below n stays on
 * the start's own cycle of E, which holds at most 2^k - n values >= n: it ends within 2^k - n + 1 applications (about
 * 2^k / n < 4 on average).  One thread per entry, no memory traffic besides ptr and the outputs, no atomics. */
int fastegnn_mmd_sample(const int64_t *ptr, int32_t B, int32_t S, uint64_t *rng, int32_t advance, int32_t *sample_nodes,
                        int32_t *sample_count, void *stream);
/* fastegnn_loss_mse_mmd where row b of sample_nodes [B,S] holds sample_count[b] <= S valid entries (the rest is never read):
 * a graph smaller than the sample contributes all its nodes, and l_rv is divided by B * S * C whatever the counts, as the
 * reference's variable-size branch does (utils/train.py:142).  A count of 0 contributes to l_vv only.  sample_count int32 [B],
 * DEVICE, must not be null unless B == 0, where nothing reads it (fastegnn_loss_mse_mmd is the form with every row full).  The
 * counts are trusted like the indices: the valid entries of a row are not range-checked.  The one thing the kernel does with a
 * count outside [0, S] is to read it as 0 or S, because a workgroup's LDS holds S rows. */
int fastegnn_loss_mse_mmd_ragged(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                                 const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                                 float weight, float *loss2, float *g_loc, float *g_vloc, void *stream);
/* The loss of a forward-only epoch (utils/train.py:104-108,163-165 with backprop=False): the same two numbers, NO gradient
 * outputs, summed over the batches of a loader on the device.  ADDITIVE export, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 *   acc  DEVICE double[3], read and advanced by this call:
 *     acc[0] += B * MSE(loc_pred, loc_t)            (the number the reference logs: train.py:107)
 *     acc[1] += B * (MSE + weight * (l_vv - l_rv))  (the full objective)
 *     acc[2] += B
 * so that acc[0] / acc[2] after the last batch is the reference's result['loss'] / result['counter'].
 * sample_nodes / sample_count as fastegnn_loss_mse_mmd_ragged (sample_count null: every row full); sample_nodes null or S == 0: the
 * MMD term is not evaluated at all (l_vv neither) and acc[1] advances by B * MSE.
 * Every sum is taken in fp64 (the differences and squares of the MSE exactly; the kernel values exp(-d / 2 sigma^2) are the fp32
 * ones of the training loss) by ONE workgroup in a fixed order: the argument list carries no workspace for workgroup partials, so
 * the fixed-order final workgroup of fastegnn_grad_sqnorm's scheme is the only one.  No atomics: two calls on the same inputs from
 * the same acc leave bit-identical acc.  Reads nothing back, synchronises nothing, capturable.  B == 0 launches nothing and leaves acc
 * as it is.  FASTEGNN_E_INVALID before any launch for: null acc, a null tensor that would be read, N < 0, B < 0, C < 0, S < 0,
 * C > 256 or S > 4096 (the ceilings of the training loss). */
int fastegnn_loss_mse_mmd_eval(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                               const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                               float weight, double *acc, void *stream);
/* The same three words for a TRAINING epoch (utils/train.py:23-179 with backprop=True), from the two numbers a training step has
 * already computed.  ADDITIVE export, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 *   loss, mse  DEVICE float: the step's objective and its plain MSE (fastegnn_loss_mse_mmd's loss2[0] and loss2[1])
 *   acc[0] += B * *mse,  acc[1] += B * *loss,  acc[2] += B       in fp64, by one thread (B * an fp32 value is exact in fp64)
 * so that an epoch's graph-weighted means cost ONE read-back after its last step.  Reads nothing back, synchronises nothing,
 * capturable.  B == 0 launches nothing.  FASTEGNN_E_INVALID before any launch for: a null pointer, B < 0. */
int fastegnn_loss_accumulate(const float *loss, const float *mse, int32_t B, double *acc, void *stream);
/* The ORDERED training loss: fastegnn_loss_mse_mmd / _ragged (sample_count null: every row full) with NO floating-point atomic.
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.  Same outputs (loss2[0..1], g_loc [N,3], g_vloc [B,3,C]), same
 * ceilings (C <= 256, S <= 4096), same reading of a count outside [0, S] as 0 or S, same zero subgradient at coincident points,
 * same divisor B * S * C of l_rv whatever the counts; the pair values exp(-d / 2 sigma^2) and the gradient terms are the fp32 ones
 * of the atomic kernels, the two loss sums are taken in fp64 and rounded once.
 *   ws  DEVICE double[ws_doubles], ws_doubles >= fastegnn_loss_ordered_ws_doubles(N, B) = G + B with G = clamp(ceil(3 N / 2048), 1,
 *       1024): written and read by this call only (the caller allocates it; nothing is allocated here).
 * ORDERING RULE -- the order of every sum is a function of (N, B, C, S) and the counts, never of arrival:
 *   MSE     workgroup x < G of 256 threads: thread t adds the squares (exact in fp64) of the elements x * 256 + t, + G * 256, ...
 *           in ascending order; the workgroup sum W is the xor butterfly (offsets 32, 16, .., 1) within each wave, then
 *           ((w0 + w1) + (w2 + w3)); it goes to ws[x].  g_loc is element-wise.
 *   MMD     one workgroup per graph b.  gV[c] is owned by thread c: a = 0 .. C-1 of the vv term (the two roles of c in the pairs
 *           (c, a) and (a, c), one after the other), then s = 0 .. count_b - 1 of the rv term.  gR[s] is owned by thread s mod 256,
 *           which takes its rows in ascending s and walks c = 0 .. C-1.  Loss terms: the owner of c adds its C vv terms, the owner
 *           of s its C rv terms, in that order, in fp64; then W as above into ws[G + b].
 *   final   ONE workgroup: thread t adds ws[t], ws[t + 256], ... below G, then W; the same over the B graph slots; loss2 is written
 *           once (no memset, no accumulation into it).
 *   g_loc at the sampled nodes: ONE plain add per address, stream-ordered behind the MSE write.  CONTRACT: the valid entries of a
 *           row of sample_nodes are distinct and the rows of different graphs name disjoint nodes (torch.randperm(n)[:S] per graph
 *           in the reference, fastegnn_mmd_sample here).  A repeated node loses all but one of its terms (no fault, not the
 *           atomic kernels' sum).
 * Two calls on the same inputs give bit-identical loss2, g_loc and g_vloc.  Capturable, no read-back, no synchronisation.
 * B == 0 writes the MSE and g_loc only.  FASTEGNN_E_INVALID before any launch for: N < 0, B < 0, C < 0, S < 0, C > 256, S > 4096,
 * null loss2 / ws, a null tensor that would be read or written, ws_doubles too small. */
size_t fastegnn_loss_ordered_ws_doubles(int32_t N, int32_t B);
int fastegnn_loss_mse_mmd_ordered(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                                  const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                                  float weight, float *loss2, float *g_loc, float *g_vloc, double *ws, size_t ws_doubles,
                                  void *stream);

/* ---- graph construction on device (datasets/simulation/dataset.py:80,96-101) ----
 * radius graph without self loops: all ordered pairs (i, j != i) with |x_i - x_j|^2 <= r^2 (fp32, each
 * operation rounded separately), grouped by i with j ascending.  Two passes so that the caller allocates:
 * _count fills the workspace (fastegnn_radius_graph_ws_bytes(N) bytes) and returns the edge count in
 * *n_edges (host; synchronises the stream), _fill writes edge_index int64 [2,E] and dist [E]. */
size_t fastegnn_radius_graph_ws_bytes(int32_t N);
int fastegnn_radius_graph_count(const float *loc, int32_t N, float r, void *ws, size_t ws_bytes, int64_t *n_edges,
                                void *stream);
int fastegnn_radius_graph_fill(const float *loc, int32_t N, float r, void *ws, size_t ws_bytes, int64_t n_edges,
                               int64_t *edge_index, float *dist, void *stream);
/* keep the `keep` shortest edges (stable: ties keep their order), in ascending length like the reference's
 * cutoff_edge; tmp: fastegnn_cutoff_tmp_bytes(E) bytes */
size_t fastegnn_cutoff_tmp_bytes(int64_t E);
int fastegnn_cutoff_edges(const int64_t *edge_index, const float *dist, int64_t E, int64_t keep, int64_t *edge_index_out,
                          float *dist_out, void *tmp, size_t tmp_bytes, void *stream);

/* The same two steps for B ragged point clouds in one call (additive at this revision).  loc [N,3] holds the clouds back to
 * back, ptr int64 [B+1] (device) their node ranges: 0 = ptr[0] <= ... <= ptr[B] = N.  Every cloud gets its own bounding box and
 * cell grid by the single-cloud rule (cell edge max(r, extent / 255), at most 256 cells per axis), so its edges -- and the
 * decision at the r boundary -- are those of fastegnn_radius_graph_* on that cloud alone, with global node ids: the list is
 * grouped by graph, inside a graph by centre in ascending id with neighbours ascending; no edge joins two graphs.  The
 * workspace (fastegnn_radius_graph_batch_ws_bytes(N, B) bytes) grows with N and B only: the points of a graph are ordered by
 * cell id inside its own range of ONE radix sort on the key (graph, cell id), and a run of cells is found by binary search in
 * that range -- there is no table over the 2^24 possible cells.
 * _count runs everything up to the per-node offsets and copies edge_ptr [B+1] (edge_ptr[b] = first edge of graph b,
 * edge_ptr[B] = E) and one status word to the host: the call's single synchronisation.  A ptr that is not as above sets
 * the status word and the call returns FASTEGNN_E_INVALID (the kernels clamp every range to [0, N], so nothing is indexed
 * outside loc).  _fill writes edge_index int64 [2,E], dist [E] and the device copy edge_ptr [B+1]; it reads nothing back.
 * N == 0 or B == 0: FASTEGNN_OK with every count zero, nothing launched.
 * FASTEGNN_E_INVALID before any device call for: a null pointer that would be used, N < 0, B < 0, r <= 0, a workspace below
 * the size above, n_edges < 0 or >= 2^31. */
size_t fastegnn_radius_graph_batch_ws_bytes(int32_t N, int32_t B);
int fastegnn_radius_graph_batch_count(const float *loc, const int64_t *ptr, int32_t N, int32_t B, float r, void *ws,
                                      size_t ws_bytes, int64_t *edge_ptr_host /* [B+1] */, void *stream);
int fastegnn_radius_graph_batch_fill(const float *loc, const int64_t *ptr, int32_t N, int32_t B, float r, void *ws,
                                     size_t ws_bytes, int64_t n_edges, int64_t *edge_index, float *dist,
                                     int64_t *edge_ptr /* device [B+1] */, void *stream);
/* Segmented cutoff: of the edges edge_ptr[b] .. edge_ptr[b+1] of graph b keep the keep_ptr[b+1] - keep_ptr[b] shortest, in
 * ascending length, equal lengths in their input order (one stable radix sort on the key (graph, distance bits)); graph b's
 * edges land at keep_ptr[b] .. of the outputs (edge_index_out int64 [2,keep_total], dist_out [keep_total], may be null).
 * edge_ptr and keep_ptr are device arrays [B+1] of prefix sums with edge_ptr[B] == E, keep_ptr[B] == keep_total and
 * keep_b <= E_b.  Reads nothing back.  tmp: fastegnn_cutoff_batch_tmp_bytes(E, B) bytes.  keep_total == 0 or B == 0 launches
 * nothing.  FASTEGNN_E_INVALID before any device call for: B < 0, E < 0, E >= 2^31, keep_total < 0 or > E, a null pointer
 * that would be used, tmp below the size above. */
size_t fastegnn_cutoff_batch_tmp_bytes(int64_t E, int32_t B);
int fastegnn_cutoff_edges_batch(const int64_t *edge_index, const float *dist, const int64_t *edge_ptr, const int64_t *keep_ptr,
                                int32_t B, int64_t E, int64_t keep_total, int64_t *edge_index_out, float *dist_out, void *tmp,
                                size_t tmp_bytes, void *stream);

/* N-body systems (datasets/nbody/dataset.py:102-113): for each of S systems of n <= 128 particles (loc [S,n,3]) the k
 * shortest ordered pairs (i, j != i) of the complete graph in ascending length (fp32 distance, each operation rounded
 * separately; equal lengths in ascending i*n+j): edge_index int64 [S,2,k] (particle ids within the system), dist [S,k]. */
int fastegnn_nbody_cutoff_edges(const float *loc, int32_t S, int32_t n, int32_t k, int64_t *edge_index, float *dist,
                                void *stream);

/* ---- mini-batch assembly from a packed dataset (the collate of torch_geometric.loader.DataLoader, main_nbody.py:93-96) ----
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 * A packed dataset holds every field of its n_frames graphs in ONE device table per field, frame after frame, with the prefix
 * sums src_node_ptr / src_edge_ptr (int64 [n_frames + 1], device) of the frames' node and edge counts; edge_index is int64
 * [2, src_edges] with node ids LOCAL to the frame.  A batch is the B frames ids[0 .. B) (int64, device; any order, repeats
 * allowed) and costs two launches whatever B is; neither call reads anything back, synchronises or allocates.
 *   _plan    node_ptr_out / edge_ptr_out int64 [B+1]: exclusive prefix sums of the chosen frames' node / edge counts (node_ptr_out
 *            is the batch's `ptr`).  One workgroup, 1024 frames per round with a running carry: any B.
 *   _gather  every output of the batch in one launch, a segmented copy (flat output element -> frame by binary search in the
 *            batch offsets -> source address; one element per lane, 64-bit indices, no atomics):
 *              dst_tables[t] [n_out, widths[t]] fp32 for t = LOC_0 .. EDGE_ATTR  (n_out = n_nodes_out, for EDGE_ATTR n_edges_out)
 *              dst_tables[LOC_MEAN] [B, widths[LOC_MEAN]] fp32   (row ids[i] of the source's [n_frames, widths[LOC_MEAN]])
 *              dst_tables[EDGE_INDEX] int64 [2, n_edges_out] = the frames' local ids + node_ptr_out[frame]
 *              batch_out int64 [n_nodes_out] = position of the node's frame in the batch (may be null: not written)
 *            src_tables / dst_tables: HOST arrays of FASTEGNN_COLLATE_TABLES device pointers in the order below, widths: HOST
 *            int32 [FASTEGNN_COLLATE_TABLES - 1] floats per row.  src_nodes / src_edges: rows of the packed node / edge tables;
 *            n_nodes_out / n_edges_out: the batch's totals, which the caller knows from its host copy of the counts and has sized
 *            the outputs by -- they must equal node_ptr_out[B] / edge_ptr_out[B].
 * The kernels clamp every id to [0, n_frames) and skip an element whose offset does not fall inside its frame's source segment,
 * so nothing is read outside [src_ptr[id], src_ptr[id+1]) or beyond the packed tables, and nothing is written beyond the totals
 * given, whatever the device arrays hold.  A table without output elements (a batch without edges) takes no part; when every
 * table is empty, or B == 0, _gather launches nothing.  FASTEGNN_E_INVALID before any launch for: B < 0, n_frames < 1, a
 * negative size, a width outside 0 .. 2^20, a null pointer that would be used. */
#define FASTEGNN_COLLATE_LOC_0 0
#define FASTEGNN_COLLATE_LOC_T 1
#define FASTEGNN_COLLATE_VEL_0 2
#define FASTEGNN_COLLATE_NODE_FEAT 3
#define FASTEGNN_COLLATE_NODE_ATTR 4
#define FASTEGNN_COLLATE_EDGE_ATTR 5
#define FASTEGNN_COLLATE_LOC_MEAN 6
#define FASTEGNN_COLLATE_EDGE_INDEX 7
#define FASTEGNN_COLLATE_TABLES 8
int fastegnn_collate_plan(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr,
                          int32_t n_frames, int64_t *node_ptr_out, int64_t *edge_ptr_out, void *stream);
int fastegnn_collate_gather(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr,
                            int32_t n_frames, int64_t src_nodes, int64_t src_edges, const int64_t *node_ptr_out,
                            const int64_t *edge_ptr_out, int64_t n_nodes_out, int64_t n_edges_out, const void *const *src_tables,
                            void *const *dst_tables, const int32_t *widths, int64_t *batch_out, void *stream);
/* The batch's SORTED graph without a sort.  ADDITIVE export, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 * fastegnn_build_csr is a stable sort by row and the frames of a batch own disjoint, ascending node ranges, so the index of the
 * batch is the frames' own indices laid end to end with an offset added.  The packed dataset keeps those, built ONCE with
 * fastegnn_build_csr (16 bytes per edge + 16 per node of device memory):
 *   g_rowptr, g_cscptr  int64 [src_nodes + 1]  position of the node's first edge in the packed row-sorted (col-keyed) edge table;
 *                       frames are contiguous: g_rowptr[src_node_ptr[f]] == src_edge_ptr[f], g_rowptr[src_nodes] == src_edges
 *   g_erow, g_col       int32 [src_edges]      row / column of every row-sorted edge, node ids LOCAL to the frame
 *   g_perm              int32 [src_edges]      position of the edge in the frame's own COO list
 *   g_csc_eid           int32 [src_edges]      position inside the frame's row-sorted list, in col-keyed order
 * ids .. n_edges_out are fastegnn_collate_gather's, node_ptr_out / edge_ptr_out fastegnn_collate_plan's.  Two launches whatever B is:
 *   1. a segmented gather over the outputs (int32, the arrays of fastegnn_graph_t with n_rows = n_src = n_nodes_out): for frame
 *      j = ids[i], no = node_ptr_out[i], eo = edge_ptr_out[i]
 *        rowptr[no + k] = g_rowptr[src_node_ptr[j] + k] - src_edge_ptr[j] + eo,  rowptr[n_nodes_out] = n_edges_out  (cscptr likewise)
 *        erow = g_erow + no,  col = g_col + no,  perm = g_perm + eo,  csc_eid = g_csc_eid + eo
 *   2. the chunk launch of fastegnn_build_csr on the assembled rowptr: chunk_row [fastegnn_chunk_rows(n_edges_out)];
 *      *n_chunks (HOST int) = n_edges_out / fastegnn_chunk_edges() + 1.
 * The result equals fastegnn_build_csr(edge_index of the batch, n_edges_out, 0, n_nodes_out, n_nodes_out, ...) element for element.
 * cscptr and csc_eid both NULL: no col-keyed index (g_cscptr / g_csc_eid may then be NULL too).  n_edges_out == 0: rowptr / cscptr
 * all zero and the one-chunk chunk_row, as build_csr writes them; the edge arrays are not touched.  No atomics, no workspace, no
 * read-back, no synchronisation.  The safety contract of _gather holds: ids clamped to [0, n_frames), an element outside its frame's
 * source segment skipped, nothing read outside the packed tables or written beyond the totals given, whatever the device arrays
 * hold.  FASTEGNN_E_INVALID before any launch for: B < 0, n_frames < 1, a negative size, n_nodes_out + 1 or n_edges_out beyond
 * int32 (build_csr's argument types), nodes or edges with B == 0, a null pointer that would be used, cscptr without csc_eid or the
 * reverse (g_cscptr / g_csc_eid alike), a col-keyed index asked for with edges but no g_cscptr. */
int fastegnn_collate_graph(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr, int32_t n_frames,
                           int64_t src_nodes, int64_t src_edges, const int64_t *node_ptr_out, const int64_t *edge_ptr_out,
                           int64_t n_nodes_out, int64_t n_edges_out, const int64_t *g_rowptr, const int32_t *g_erow,
                           const int32_t *g_col, const int32_t *g_perm, const int64_t *g_cscptr, const int32_t *g_csc_eid,
                           int32_t *rowptr, int32_t *erow, int32_t *col, int32_t *perm, int32_t *cscptr, int32_t *csc_eid,
                           int32_t *chunk_row, int32_t *n_chunks, void *stream);

/* ---- streaming a packed dataset of EQUAL-SIZED frames (the N-body sets: every frame n particles and the same top-k pairs) ----
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.  When every frame holds nodes_per_frame nodes and
 * edges_per_frame edges, every full batch has the same shapes and a frame's place in a table is a multiplication: the batch lives in
 * buffers allocated once, its order is drawn on the device, and a batch is two launches (three with its sorted graph) that are the
 * same every time.  Neither call reads anything back, synchronises or allocates; both are capturable.
 *
 * _draw  the frame numbers of the next batch.  state DEVICE uint64[4] = {seed, epoch, cursor, reserved}.  With nb = n_frames / B
 *   (full batches only; the n_frames % B frames left over differ per epoch under shuffle) and c = cursor % nb:
 *     ids_out[i] = perm(c * B + i)   for i < B
 *   shuffle == 0: perm is the identity.  Otherwise perm is perm_b of fastegnn_mmd_sample above, bit for bit (mix64, mix32, eight
 *   Feistel rounds over 2^k >= n_frames, cycle walking), with n := n_frames, counter := epoch and b := 0x5354524D -- a fixed tag, so
 *   that a stream and an MMD sampler with equal seeds do not draw with the same keys.  One epoch visits nb * B distinct frames.
 *   advance != 0: after every id is written, cursor = c + 1; when that reaches nb, cursor = 0 and epoch += 1.  ONE launch of one
 *   workgroup: every thread reads the state, a workgroup barrier follows the last id (rounds of 1024 ids for larger B), then thread
 *   0 writes the two words -- a draw sees one consistent state, and replays of a captured draw walk on through the epochs.
 *   Whatever the state words hold, every id written is in [0, n_frames).  `reserved` is neither read nor written.
 *   FASTEGNN_E_INVALID before any launch for: a null pointer, B < 1, n_frames < B.
 *
 * _gather_uniform  the batch of the B frames ids[0 .. B) in ONE launch over a job table: no offset arrays, no binary search, no
 *   plan launch.  src_tables / dst_tables / widths as fastegnn_collate_gather; src_nodes / src_edges must equal n_frames *
 *   nodes_per_frame / n_frames * edges_per_frame.  Element e of a table with w floats per row and `count` rows per frame belongs
 *   to batch slot f = e / (count * w); its source element is clamp(ids[f]) * count * w + (e - f * count * w), the id clamped to
 *   [0, n_frames).  LOC_MEAN has one row per frame.  EDGE_INDEX (int64 [2, B * edges_per_frame], row r of the source at
 *   r * src_edges) adds f * nodes_per_frame.  `ptr`, `batch` and the edge offsets of the batch are NOT written: they never change
 *   for a uniform stream and the caller writes them once.
 *   With rowptr != NULL the same launch assembles the batch's sorted graph from the six packed tables of fastegnn_collate_graph,
 *   by its formulas with no = f * nodes_per_frame, eo = f * edges_per_frame and src_edge_ptr[j] = j * edges_per_frame;
 *   rowptr[B * nodes_per_frame] = cscptr[..] = B * edges_per_frame; a second launch (the chunk launch of fastegnn_build_csr)
 *   writes chunk_row, and *n_chunks (HOST int) = B * edges_per_frame / fastegnn_chunk_edges() + 1.  cscptr / csc_eid both NULL: no
 *   col-keyed index.  rowptr == NULL: no graph, the graph arguments are not looked at and *n_chunks is not written.
 *   edges_per_frame == 0: the edge jobs take no part, rowptr / cscptr are all zero and chunk_row is the one-chunk form.
 *   Access width, chosen per job on the host: 16 bytes per lane when the job's per-frame segment length in bytes and both base
 *   addresses are multiples of 16, 8 bytes when they are multiples of 8, else one element per lane (row 1 of a packed edge_index
 *   is 16-byte aligned only when src_edges is even); the int64 -> int32 pointer jobs are one element per lane.  A lane's vector
 *   never straddles two frames.  Several loads are in flight before the stores; beyond the block cap the workgroups stride over
 *   the tiles.  The safety contract of _gather holds: ids clamped, nothing read outside the packed tables, nothing written beyond
 *   B * the counts, whatever ids holds.
 *   FASTEGNN_E_INVALID before any launch for: B < 1, n_frames < 1, a negative count, src_nodes / src_edges that are not n_frames
 *   times the counts, a width outside 0 .. 2^20, a null pointer that would be used, a batch beyond the int32 sizes of build_csr
 *   when a graph is asked for, cscptr without csc_eid or the reverse, a col-keyed index asked for with edges but no g_cscptr /
 *   g_csc_eid.  The packed graph tables are looked at only when edges_per_frame > 0 (a dataset without edges holds empty ones). */
int fastegnn_collate_draw(uint64_t *state, int32_t B, int32_t n_frames, int32_t shuffle, int32_t advance, int64_t *ids_out,
                          void *stream);
int fastegnn_collate_gather_uniform(const int64_t *ids, int32_t B, int32_t n_frames, int64_t nodes_per_frame,
                                    int64_t edges_per_frame, int64_t src_nodes, int64_t src_edges, const void *const *src_tables,
                                    void *const *dst_tables, const int32_t *widths, const int64_t *g_rowptr, const int32_t *g_erow,
                                    const int32_t *g_col, const int32_t *g_perm, const int64_t *g_cscptr, const int32_t *g_csc_eid,
                                    int32_t *rowptr, int32_t *erow, int32_t *col, int32_t *perm, int32_t *cscptr, int32_t *csc_eid,
                                    int32_t *chunk_row, int32_t *n_chunks, void *stream);

/* ---- mini-batch assembly from device-resident trajectories (datasets/simulation/dataset.py:71-93, datasets/protein/dataset.py:81-173) ----
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 * A trajectory dataset keeps the POSITIONS, not the graphs made of them: pos fp32 [pos_rows, 3] holds every trajectory frame after
 * frame (trajectory t: rows traj_row0[t] + f * traj_n[t] .. of frame f < traj_T[t]); kind / kind_scaled fp32 [kind_rows] hold the
 * particle kinds of trajectory t (and kind / max kind) at traj_kind0[t] ..; traj_row0 / traj_n / traj_T / traj_kind0 are int64
 * [n_traj], samples int64 [n_samples, 2] = (trajectory, start frame), all on the device.  A batch is the B samples ids[0 .. B)
 * (int64, device; any order, repeats allowed); slot i of it is the cloud of n nodes of sample ids[i] = (t, f):
 *   loc_0 = pos[f], vel_0 = pos[f+1] - pos[f], loc_t = pos[f+delta_t], node_feat = [|vel_0|, kind_scaled], node_attr = kind.
 * Its node side is three launches whatever B is; none reads anything back, synchronises, allocates or uses an atomic, and the only
 * workspace is the slot table.
 *   _plan    ptr_out int64 [B+1]: exclusive prefix sums of the samples' node counts (the batch's `ptr`); slots_out int64
 *            [B, FASTEGNN_TRAJ_SLOT_WORDS]: first source row in pos of frames f, f+1, f+delta_t and first row in kind.  One workgroup,
 *            1024 samples per round with a running carry: any B.
 *   _gather  ONE launch over the n_nodes_out nodes (one node per lane, tiles of 1024; a tile finds the slots it touches by binary
 *            search in ptr, a tile inside one slot searches nothing per node): loc_0, loc_t, vel_0 fp32 [n,3], node_feat [n,2],
 *            node_attr [n,1], batch_out int64 [n] = the node's slot.  vel_0 is one fp32 subtraction per component;
 *            node_feat[:,0] = sqrt((vx*vx + vy*vy) + vz*vz) with every operation rounded to fp32 by itself (no fused multiply-add)
 *            and a correctly rounded square root; the rest are copies.  n_nodes_out is the caller's, from its host copy of the node
 *            counts, and must equal ptr[B].
 *   _mean    one workgroup of 256 threads per slot: loc_mean fp32 [B,3,C], every [b,k,:] = the sum of the slot's loc_0[:,k] in fp64
 *            (thread t adds nodes t, t+256, .. in ascending order, the 256 partial sums are added pairwise over strides 128 .. 1: an
 *            order that depends on the node count alone), divided by n in fp64, rounded to fp32, repeated C times.  A slot without
 *            nodes gives 0.
 * _plan clamps sample ids to [0, n_samples), trajectory numbers to [0, n_traj) and frame numbers (f, f+1, f+delta_t each) to [0, T);
 * _gather and _mean skip a slot whose source rows do not lie inside [0, pos_rows) / [0, kind_rows): nothing is read outside the
 * tables and nothing is written beyond n_nodes_out rows (B rows of loc_mean), whatever the device arrays hold.  B == 0 or
 * n_nodes_out == 0: _gather launches nothing.  FASTEGNN_E_INVALID before any launch for: B < 0, n_samples < 1, n_traj < 1,
 * delta_t < 0, a negative size, C outside 1 .. 2^20, nodes asked for from an empty table, a null pointer that would be used. */
#define FASTEGNN_TRAJ_SLOT_WORDS 4
int fastegnn_traj_plan(const int64_t *ids, int32_t B, const int64_t *samples, int64_t n_samples, const int64_t *traj_row0,
                       const int64_t *traj_n, const int64_t *traj_T, const int64_t *traj_kind0, int32_t n_traj, int32_t delta_t,
                       int64_t *ptr_out, int64_t *slots_out, void *stream);
int fastegnn_traj_gather(const int64_t *ptr, const int64_t *slots, int32_t B, int64_t n_nodes_out, const float *pos, int64_t pos_rows,
                         const float *kind, const float *kind_scaled, int64_t kind_rows, float *loc_0, float *loc_t, float *vel_0,
                         float *node_feat, float *node_attr, int64_t *batch_out, void *stream);
int fastegnn_traj_mean(const int64_t *ptr, const int64_t *slots, int32_t B, const float *pos, int64_t pos_rows, int32_t C,
                       float *loc_mean, void *stream);

/* ---- rollouts: the state update between two forwards of a model that is fed its own prediction (fastegnn_amd/rollout.py) ----
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.  The project's own semantics (the reference has no rollout).
 * A rollout of the B samples ids[0 .. B) = (trajectory t, start frame f) of the tables above, with stride delta_t >= 1, starts from the
 * node tensors of fastegnn_traj_gather / _mean; step k = 0, 1, .. hands the model the state and gets x_new fp32 [n_nodes,3], its
 * prediction of frame f + (k+1) delta_t.  The state is then advanced by TWO launches whatever B is; none reads anything back,
 * synchronises, allocates or uses an atomic, and both are capturable:
 *   _advance  ONE launch over the n_nodes nodes, one node per lane, tail masked; per component
 *               vel = (x_new - loc) * (1.0f / delta_t)   one fp32 subtraction, then one fp32 multiplication, no fused multiply-add
 *               loc = x_new                              (in place: `loc` holds x_cur on entry; x_new must not alias it)
 *             and node_feat[:,0] = sqrt((vx*vx + vy*vy) + vz*vz) by _gather's rule; node_feat[:,1] is not touched.  `record`, when not
 *             null, is fp32 [n_nodes,3] and receives x_new as it came.  A NON-FINITE component of x_new does not enter the state: loc
 *             keeps its value, the vel component is 0, and the int32 word `flag` (device or host-mapped, fastegnn_host_words_alloc)
 *             gets a plain store of the constant 1 -- an all-finite call leaves it alone; `record` still gets the raw value.
 *   _graph    one workgroup of 256 threads per graph b (nodes ptr[b] .. ptr[b+1]): loc_mean fp32 [B,3,C] of `loc` by _mean's rule (the
 *             bits fastegnn_traj_mean gives on the same rows) and, in the same pass, when `sse` is not null,
 *               sse[b] = sum over the graph's nodes of (dx*dx + dy*dy) + dz*dz,  d = (double)x_new - (double)pos[truth_rows[b] + i]
 *             in fp64, every operation rounded by itself, summed in _mean's order (thread t takes nodes t, t+256, .., then the pairwise
 *             tree).  sse[b] = NaN where truth_rows[b] < 0 (no truth frame), where truth_rows[b] .. + n does not lie inside
 *             [0, pos_rows), or where the graph has no node.  A graph whose node range does not lie inside [0, n_nodes) counts as
 *             empty (loc_mean 0).  sse null: x_new, pos and truth_rows are not read.  The caller passes row k of its [steps,B] tables.
 * and once per rollout
 *   _plan     ONE launch: truth_rows int64 [steps,B], [k,b] = the first row in pos of frame f + (k+1) delta_t of slot b, or -1 where that
 *             frame is not below T.  Sample ids, trajectory numbers and start frames are clamped as fastegnn_traj_plan clamps them;
 *             nothing is uploaded.
 * Nothing is read outside the tables and nothing is written beyond n_nodes rows (B rows of loc_mean / sse, steps * B words of
 * truth_rows), whatever the device arrays hold.  FASTEGNN_E_INVALID before any launch for: a negative size, steps < 1, delta_t < 1,
 * n_samples < 1, n_traj < 1, C outside 1 .. 2^20, a null pointer that would be used (`flag` always). */
int fastegnn_rollout_plan(const int64_t *ids, int32_t B, const int64_t *samples, int64_t n_samples, const int64_t *traj_row0,
                          const int64_t *traj_n, const int64_t *traj_T, int32_t n_traj, int32_t delta_t, int32_t steps,
                          int64_t *truth_rows, void *stream);
int fastegnn_rollout_advance(const float *x_new, int64_t n_nodes, int32_t delta_t, float *loc, float *vel, float *node_feat,
                             float *record, int32_t *flag, void *stream);
int fastegnn_rollout_graph(const int64_t *ptr, int32_t B, const float *loc, const float *x_new, int64_t n_nodes, const float *pos,
                           int64_t pos_rows, const int64_t *truth_rows, int32_t C, float *loc_mean, double *sse, void *stream);

/* ---- rigid motions: trajectory batches and rollouts in a rotated and shifted frame (datasets/simulation/dataset.py:71-77,
 *      datasets/protein/dataset.py:131-142: the reference moves its test partitions BEFORE it builds their graphs) ----
 * ADDITIVE exports, found by symbol: FASTEGNN_ABI_VERSION stays 108.
 * THE RULE.  A motion is 12 fp32 values: R row-major (9), then t (3).  For a row vector p
 *     q[j] = ((p[0]*R[0][j] + p[1]*R[1][j]) + p[2]*R[2][j])        j = 0, 1, 2
 *     moved position = q + t          moved velocity = q  (no t)
 * Every multiplication and every addition is fp32 and rounded by itself (no fused multiply-add: the statements are compiled with
 * contraction off, as _gather's speed is): the reference's x @ R (+ t) in one fixed evaluation order, which elementwise torch
 * operations reproduce bit for bit on either device (fastegnn_amd.data.apply_motion).  With has_t == 0 the `+ t` is NOT executed -- it
 * is not an addition of +0.0f, which would turn -0.0 into +0.0 -- and the three t values are not used.
 * `motion` is fp32 [B,12] on the device, one row per SLOT of the batch (row i moves the cloud of ids[i]); it is read at the slot index,
 * which is below B by construction, never through an index that comes from the data.
 *   _traj_gather_moved   fastegnn_traj_gather with the motion applied in the same launch (same tiling; a tile inside one slot loads
 *                        its 12 values once): loc_0 = move(pos[f]), loc_t = move(pos[f+delta_t]), vel_0 = rotate(pos[f+1] - pos[f]) --
 *                        the difference first, as the reference has it --, node_feat[:,0] = the speed of the ROTATED velocity by
 *                        _gather's rule; node_feat[:,1], node_attr and batch_out as _gather writes them; the same clamps and skips.
 *                        loc_mean of a moved batch is _mean's rule over the moved loc_0, which fastegnn_rollout_graph(ptr, B, loc_0,
 *                        NULL, n, NULL, 0, NULL, C, loc_mean, NULL, stream) computes from the [n,3] tensor: four launches whatever B.
 *   _rollout_graph_moved fastegnn_rollout_graph with the truth row moved, in fp32 by the rule, before the fp64 difference:
 *                        d = (double)x_new - (double)move(pos[truth_rows[b] + i]); the summation order, the NaN rules and loc_mean
 *                        are _rollout_graph's (loc_mean has the bits of the unmoved call on the same `loc`).  sse null: motion is
 *                        not read.
 * FASTEGNN_E_INVALID before any launch for what _traj_gather / _rollout_graph refuse, and for a null `motion` that would be read. */
int fastegnn_traj_gather_moved(const int64_t *ptr, const int64_t *slots, int32_t B, int64_t n_nodes_out, const float *pos,
                               int64_t pos_rows, const float *kind, const float *kind_scaled, int64_t kind_rows, float *loc_0,
                               float *loc_t, float *vel_0, float *node_feat, float *node_attr, int64_t *batch_out, const float *motion,
                               int32_t has_t, void *stream);
int fastegnn_rollout_graph_moved(const int64_t *ptr, int32_t B, const float *loc, const float *x_new, int64_t n_nodes, const float *pos,
                                 int64_t pos_rows, const int64_t *truth_rows, int32_t C, float *loc_mean, double *sse,
                                 const float *motion, int32_t has_t, void *stream);

/* ---- exchange steps of the sharded path (the reference has no distributed code) ----
 * RCCL collectives behind the C ABI: every call is enqueued on `stream` (ordered with the stage kernels, capturable
 * into a HIP graph) and returns at once.  RCCL is bound at run time (dlopen; FASTEGNN_E_NODEVICE when absent).
 * Bring-up: rank 0 calls fastegnn_comm_unique_id, the caller distributes the fastegnn_comm_unique_id_bytes() bytes by
 * any out-of-band means, every rank calls fastegnn_comm_init.  One communicator per process and device. */
typedef struct fastegnn_comm fastegnn_comm_t;
int32_t fastegnn_comm_unique_id_bytes(void);
int fastegnn_comm_unique_id(void *id);
int fastegnn_comm_init(fastegnn_comm_t **comm, const void *id, int32_t rank, int32_t world);
int fastegnn_comm_destroy(fastegnn_comm_t *comm);
int32_t fastegnn_comm_rank(const fastegnn_comm_t *comm);
int32_t fastegnn_comm_world(const fastegnn_comm_t *comm);
/* buf <- sum over ranks (xsum [B,4]; poolV|poolX; g_Bc|g_Zp; the flat parameter-gradient buffer) */
int fastegnn_comm_all_reduce(fastegnn_comm_t *comm, float *buf, size_t n, void *stream);
/* QX [Npad,68] of every rank -> QX_src [W*Npad,68] ("allgather" table exchange) and its transpose */
int fastegnn_comm_all_gather(fastegnn_comm_t *comm, const float *in, float *out, size_t n_per_rank, void *stream);
int fastegnn_comm_reduce_scatter(fastegnn_comm_t *comm, const float *in, float *out, size_t n_per_rank, void *stream);
/* halo exchange: send_rows[r] rows of row_floats floats go to rank r (from `send`, in rank order), recv_rows[r] rows
 * arrive from rank r (into `recv`, in rank order); the backward swaps the two count arrays.  HOST arrays [world]. */
int fastegnn_comm_all_to_all_v(fastegnn_comm_t *comm, const float *send, const int64_t *send_rows, float *recv,
                               const int64_t *recv_rows, int32_t row_floats, void *stream);
/* ghost-row pack / unpack of the halo exchange: out[r,:] = table[ids[r],:] (width % 4 == 0);  table[ids[r],:] += rows[r,:] */
int fastegnn_gather_rows(const float *table, const int64_t *ids, int64_t n, int32_t width, float *out, void *stream);
int fastegnn_scatter_add_rows(float *table, const int64_t *ids, int64_t n, int32_t width, const float *rows, void *stream);

/* ---- the WIDE path: 64 < hidden_nf <= 256 (models/FastEGNN.py:28-99 takes any hidden_nf; main_nbody.py:27 --dim_hidden) ----
 * The fused stage kernels above are built on 64-wide tiles.  A wider model runs unfused: the op sequence of
 * models/FastEGNN.py:102-223 with every hidden-sized tensor op as ONE of the launches below (fastegnn_amd/wide.py; autograd
 * composes the backward from the _dx / _dw / _backward entry points).  fp32-grade arithmetic (the GEMMs as bf16x3 splits on the
 * matrix pipe, csrc/wide_gemm.h), row-major contiguous operands, int64 indices as the reference's edge_index / data['batch']
 * hold them.  ABI revision 104; revision 106 added the fused activation arguments of the three linear entry points:
 * act_kind = FASTEGNN_ACT_* makes X the PRE-activation of the Linear's input (nn.Sequential(Linear, act, Linear),
 * models/FastEGNN.py:41-99: act(X) is formed in the kernel and never stored), FASTEGNN_ACT_NONE takes X as is.
 *   linear      out[M,O] = (base ? base : 0) + act(X)[M,K] . W[:, c0:c0+K]^T + bias -- nn.Linear; a Linear over a torch.cat of
 *               inputs is the sum of these calls over the weight's column blocks (W row stride ldw), chained through `base`
 *   linear_dx   dX[M,K] (+)= (G[M,O] . W[:, c0:c0+K]) * act'(Z[M,K])   -- Z NULL: no activation factor; with Z the result is the
 *               gradient of the pre-activation Z that `linear` took
 *   linear_dw   dW[:, c0:c0+K] += G^T act(X),  db += column sums of G (either may be NULL); fp32 atomics over row ranges
 *               (linear_dw_ordered below: the same sums in a fixed order)
 *   head_dx / head_dw   the backward of the first Linear of a scalar head s = act(X W1^T + b1) . w2^T (coord_mlp_*, gravity_mlp:
 *               models/FastEGNN.py:55-99) from the head's output gradient gs[M]: G[m,o] = gs[m] w2[o] act'(Zc[m,o]) is formed in
 *               the kernels from the stored pre-activation Zc and never written; O (hidden width) a multiple of 4, O and K >= 9;
 *               head_dw also returns the second Linear's weight gradient dw2[o] += sum_m gs[m] act(Zc[m,o]) (may be NULL)
 *   head_forward  Zc = act_x(X) W1^T + b1 (stored) and s = act(Zc) . w2 + b2: with 9 .. 128 hidden units s comes out of the first
 *               GEMM's accumulators (no pass over Zc), otherwise from a second launch
 *   act         y = act_fn(z), kind = FASTEGNN_ACT_*, p = its parameter;  act_backward  dz = dy * act_fn'(z)
 *   gather_add  out[m,:] = (base ? base[m,:] : 0) + X[idx[m],:]      -- node_feat[row], virtual_node_feat[data_batch]
 *   gather2     out[m,:] = (base) + P[i1[m],:] + (Q ? Q[i2[m],:] : 0) + feat[m,0:nf] . Wf[:, c0:c0+nf]^T  (feat may be NULL, nf <= 8)
 *               -- the first Linear of edge_model over cat[h[row], h[col], radial, edge_attr] (models/FastEGNN.py:102-108) in one
 *               write-only pass, given the node-sized products P and Q; edge_mode_virtual (:111-119) in the same form
 *   scatter_add table[idx[m],:] += rows[m,:]                         -- unsorted_segment_sum / global_mean_pool sums (atomics;
 *               runs of equal targets are summed in registers first)
 *   act_scatter y = act_fn(z) stored AND table[idx[m],:] += y[m,:] in one pass (edge_mlp's output and its segment sum for node_model,
 *               models/FastEGNN.py:108, 156; edge_mlp_virtual's and node_model_virtual's pool, :119, 170);
 *               act_scatter_backward  dz = ((g_y ? g_y : 0) + g_table[idx]) * act_fn'(z)
 *   scatter_add_perm  table[idx_sorted[m],:] += rows[perm[m],:]      -- the same for an index in any order, given the permutation
 *               that sorts it (idx_sorted = idx[perm], once per graph): the edge COLUMN sums of the backward as runs
 *   rowscale    Y[m,:] = X[m,:] * s[m];  rowdot  out[m] = <A[m,:], B[m,:]>   -- gates, 1/count of the segment means */
int fastegnn_wide_linear(const float *X, int64_t M, int32_t K, const float *W, int32_t ldw, int32_t c0, const float *bias,
                         const float *base, float *out, int32_t O, int32_t act_kind, float act_p, void *stream);
int fastegnn_wide_linear_dx(const float *G, int64_t M, int32_t O, const float *W, int32_t ldw, int32_t c0, int32_t K, float *dX,
                            int32_t accumulate, const float *Z, int32_t act_kind, float act_p, void *stream);
int fastegnn_wide_linear_dw(const float *G, const float *X, int64_t M, int32_t O, int32_t K, float *dW, int32_t ldw, int32_t c0,
                            float *db, int32_t act_kind, float act_p, void *stream);
int fastegnn_wide_head_dx(const float *gs, const float *w2, const float *Zc, int64_t M, int32_t O, const float *W, int32_t ldw,
                          int32_t c0, int32_t K, float *dX, int32_t accumulate, int32_t kind, float p, void *stream);
int fastegnn_wide_head_dw(const float *gs, const float *w2, const float *Zc, const float *X, int64_t M, int32_t O, int32_t K, float *dW,
                          int32_t ldw, int32_t c0, float *db, float *dw2, int32_t kind, float p, int32_t x_kind, float x_p, void *stream);
int fastegnn_wide_head_forward(const float *X, int64_t M, int32_t K, const float *W1, int32_t ldw, int32_t c0, const float *b1,
                               const float *w2, const float *b2, float *Zc, float *s, int32_t O, int32_t kind, float p, int32_t x_kind,
                               float x_p, void *stream);
int fastegnn_wide_act(const float *z, int64_t n, int32_t kind, float p, float *y, void *stream);
int fastegnn_wide_act_backward(const float *z, const float *dy, int64_t n, int32_t kind, float p, float *dz, void *stream);
int fastegnn_wide_gather_add(const float *X, const int64_t *idx, int64_t M, int32_t W, const float *base, float *out, void *stream);
int fastegnn_wide_gather2(const float *P, const int64_t *i1, const float *Q, const int64_t *i2, const float *feat, int32_t nf,
                          const float *Wf, int32_t ldw, int32_t c0, const float *base, float *out, int64_t M, int32_t W, void *stream);
int fastegnn_wide_scatter_add(float *table, const int64_t *idx, int64_t M, int32_t W, const float *rows, void *stream);
int fastegnn_wide_act_scatter(const float *z, const int64_t *idx, int64_t M, int32_t W, int32_t kind, float p, float *y, float *table,
                              void *stream);
int fastegnn_wide_act_scatter_backward(const float *z, const int64_t *idx, int64_t M, int32_t W, int32_t kind, float p, const float *g_y,
                                       const float *g_table, float *dz, void *stream);
int fastegnn_wide_scatter_add_perm(float *table, const int64_t *idx_sorted, const int64_t *perm, int64_t M, int32_t W, const float *rows,
                                   void *stream);
int fastegnn_wide_rowscale(const float *X, const float *s, int64_t M, int32_t W, float *Y, void *stream);
int fastegnn_wide_rowdot(const float *A, const float *B, int64_t M, int32_t W, float *out, void *stream);

/* ---- the ORDERED forms of the wide path's sums (additive exports, revision unchanged) ----
 * Every other wide entry point gives each output element to one thread that adds in a fixed order.  The sums above that do not --
 * scatter_add, scatter_add_perm, act_scatter, linear_dw, head_dw: fp32 atomics in arrival order -- have the counterparts below, which
 * use NO floating-point atomics: their results depend on (inputs, shapes) only, bit for bit, on any device, grid or occupancy.  The
 * caller passes a workspace of at least the *_ws_bytes query, 16-byte aligned; its contents before and after a call mean nothing.  As
 * everywhere in this header the library allocates nothing and never synchronises.
 *
 * segment_sum_ordered   table[t,:] = sum over the rows m with idx_sorted[m] == t of r(m), r(m) = act(rows[p(m),:]), p(m) = perm ?
 *     perm[m] : m.  idx_sorted must be non-decreasing (a stable sort of an index plus the permutation that sorts it, or an index
 *     that is sorted already with perm NULL).  act_kind = FASTEGNN_ACT_NONE and y NULL: rows as they are; act_kind >= 0: rows are
 *     pre-activations, y[p(m),:] = act(rows[p(m),:]) is stored as well (the ordered act_scatter).  Rows of the table that idx_sorted
 *     does not name are left as they were; a named row is OVERWRITTEN with its sum (callers zero-fill, so this is the += of
 *     scatter_add on a zeroed table).  The order, per column: rps = 16, doubled while rps < 256 and ceil(M / rps) * W > 2^21.  Slot g
 *     holds positions [g rps, min((g+1) rps, M)) of the sorted order.  Within a slot the terms of a run of equal targets are added
 *     one by one in ascending position onto 0.f (fp32).  A run inside one slot is that sum.  A run over the slots g0 < .. < g1 is
 *     ((s(g0) + s(g0+1)) + ..) + s(g1), s(g) the run's sum within slot g.  With a stable sort ascending position is input order.
 *     Workspace: ceil(M / rps) * 2 * W floats.
 * linear_dw_ordered / head_dw_ordered   the arguments and the += semantics of linear_dw / head_dw.  The rows are cut into nz
 *     consecutive ranges, a function of (M, O, K) alone:
 *       O > 8 and K > 8:   ns = min(ceil(512 / (ceil(O/128) ceil(K/128))), ceil(M / 256), floor(16 MiB / (4 (O K + 2 O)))), at least 1;
 *                          rows = ceil(M / ns) rounded up to a multiple of 32; nz = ceil(M / rows)
 *       otherwise:         ns = min(ceil(M / 512), 512, floor(4 MiB / (4 (O K + O)))), at least 1; rows = ceil(M / ns); nz = ceil(M / rows)
 *     Each range's partial dW block, db and dw2 are stored to its own slab of the workspace (fp32; within a range the kernels add in
 *     a fixed order of their own), then ONE thread per element adds the nz partials in ascending range order in double, rounds once to
 *     fp32 and adds that to dW[o, c0 + k] / db[o] / dw2[o].  Workspace: nz (O K + 2 O) floats, nz (O K + O) in the small forms. */
size_t fastegnn_wide_segment_sum_ws_bytes(int64_t M, int32_t W);
int fastegnn_wide_segment_sum_ordered(float *table, const int64_t *idx_sorted, const int64_t *perm, int64_t M, int32_t W, const float *rows,
                                      int32_t act_kind, float act_p, float *y, float *ws, size_t ws_bytes, void *stream);
size_t fastegnn_wide_linear_dw_ws_bytes(int64_t M, int32_t O, int32_t K);
int fastegnn_wide_linear_dw_ordered(const float *G, const float *X, int64_t M, int32_t O, int32_t K, float *dW, int32_t ldw, int32_t c0,
                                    float *db, int32_t act_kind, float act_p, float *ws, size_t ws_bytes, void *stream);
int fastegnn_wide_head_dw_ordered(const float *gs, const float *w2, const float *Zc, const float *X, int64_t M, int32_t O, int32_t K,
                                  float *dW, int32_t ldw, int32_t c0, float *db, float *dw2, int32_t kind, float p, int32_t x_kind,
                                  float x_p, float *ws, size_t ws_bytes, void *stream);

/* ---- per-kernel timing with HIP events recorded on the launch stream (bench.py) ----
 * enable(1) brackets every kernel launch of this library with two events; collect() waits for
 * them and returns, per kernel id in [0, fastegnn_profile_kernels()), the summed duration in ms
 * and the launch count since the previous collect().  Not thread-safe; off by default. */
int fastegnn_profile_enable(int32_t on);
int32_t fastegnn_profile_kernels(void);
const char *fastegnn_profile_name(int32_t id);
int fastegnn_profile_collect(double *total_ms, int64_t *launches);

/* ---- diagnostics (used by tests/ only) ----
 * Y[j][o] = sum_k A[o][k] X[j][k] for one 16-row tile through the MFMA image path (A = W or W^T,
 * W 64x64 row-major);  dW += G^T T, db += colsum(G) over M rows of 64. */
int fastegnn_selftest_gemm(const float *W, const float *X, float *Y, int32_t transposed, void *stream);
/* same through a row-major split image in LDS (one copy serves W and W^T: ds_read_b64 / ds_read_b64_tr_b16);
 * mode 0: bf16x3 products, 1: one bf16 product of the rounded operands */
int fastegnn_selftest_rm(const float *W, const float *X, float *Y, int32_t transposed, int32_t mode, void *stream);
/* transposing tile sum of the backward kernels (common.h jreduce16): X one 16x64 tile; out[16 q + j] = sum over the 16
 * rows of X[row][16 (j >> 2) + 4 q + (j & 3)] */
int fastegnn_selftest_jreduce(const float *X, float *out, void *stream);
/* X [64] -> out [128]: the kernels' cross-lane sums of one wave: out[l] = sum over the lanes l % 16 + 16 q (v_permlane16_swap /
 * v_permlane32_swap), out[64 + l] = sum over the 16 lanes of l's row (DPP rotations) */
int fastegnn_selftest_lane_sums(const float *X, float *out, void *stream);
/* `iters` dependent 64x64 MFMA layers per wave (mode bit0: SiLU between layers, bit1: image from
 * global memory instead of LDS); out receives one 16x64 tile.  Calibrates the MFMA building block. */
int fastegnn_selftest_chain(const float *wimg, float *out, int32_t iters, int32_t mode, int32_t waves, int32_t grid,
                            void *stream);
/* same chain on the 3-way bf16 split path (W 64x64 row-major fp32, X one 16x64 tile); mode bit2: one
 * layer, raw output (accuracy check against fp64). */
int fastegnn_selftest_chain_bf3(const float *W, const float *X, float *out, int32_t iters, int32_t mode, int32_t waves,
                                int32_t grid, void *stream);
int fastegnn_selftest_wgrad(const float *G, const float *T, int32_t M, float *dW, float *db, float *slab,
                            void *stream);
/* host-only: slab planning of a weight-gradient batch (n_jobs jobs of M[k] rows x nb[k] slices, then n_slab_jobs jobs of
 * slabs_each caller-written slabs) under a split limit and a slab share; nsplit_out[k] = partial slabs per slice of job k */
int fastegnn_selftest_wgrad_plan(const int64_t *M, const int32_t *nb, int32_t n_jobs, int32_t n_slab_jobs, int32_t slabs_each,
                                 int32_t max_split, int32_t slab_cap, int32_t *nsplit_out);
/* Host-only self-test of the open batch's overwrite guard (a stage must not write what a queued, not yet contracted job reads) */
int fastegnn_selftest_wgrad_guard(int64_t M, int64_t probe_off, int64_t probe_n);
/* HBM streaming calibration: mode 0 reads src (n_floats, multiple of 4), 1 copies src -> dst, 2 writes dst */
int fastegnn_selftest_stream(const float *src, float *dst, size_t n_floats, int32_t mode, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTEGNN_HIP_H */
