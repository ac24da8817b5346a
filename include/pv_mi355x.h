/*
 * pv_mi355x.h -- C ABI of the MI355X (gfx950) forward path for PyTorchVideo-style models.
 *
 * The reference (facebookresearch/pytorchvideo) has no native code and therefore no FFI
 * of its own; every FLOP on its hot path is an ATen op called from Python.  The entry
 * points below are what a reference-side binding (ctypes) binds for
 * the deploy form of an `EfficientBlockBase` (pytorchvideo/accelerator/efficient_blocks/
 * efficient_block_base.py:8-35) registered under the target device "mi355x" in
 * EFFICIENT_BLOCK_TRANSMUTER_REGISTRY (pytorchvideo/accelerator/deployment/common/
 * model_transmuter.py:16).  Each function cites the reference op graph it replaces.
 *
 * Conventions
 *   - plain pointers (device memory) + sizes in POD descriptors; no torch types.
 *   - activations are channels-last: voxel (b,t,h,w) of a tensor lives at
 *         ptr + b*bs + ((t*H + h)*W + w)*ld          (element units)
 *     and carries `round_up(C,8)` channels, the padding channels being exactly 0.
 *     Token tensors (B,N,C) are the same thing with T=H=1, W=N.
 *   - dtype is PV_F32 or PV_BF16 for activations and packed weights; all accumulation,
 *     BN/bias epilogues, softmax, LayerNorm statistics are fp32.
 *   - every call is asynchronous on `stream`, never allocates, never synchronises and is
 *     safe under hipGraph capture.  Return value: PV_OK or a negative pv_status.
 */
#ifndef PV_MI355X_H_
#define PV_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pv_stream_t; /* hipStream_t */

enum pv_status {
  PV_OK = 0,
  PV_ERR_UNSUPPORTED = -1, /* shape/option not implemented by the kernels            */
  PV_ERR_INVALID = -2,     /* inconsistent descriptor (reference raises RuntimeError) */
  PV_ERR_HIP = -3          /* a HIP runtime call failed; see pv_last_error()          */
};

enum pv_dtype { PV_F32 = 0, PV_BF16 = 1, PV_U8 = 2 /* source of pv_ingest_ncdhw only: decoded video frames */,
                PV_U16 = 3 /* source of the YUV 4:2:0 ingest only: 16-bit little-endian samples (pv_yuv16_views) */ };

enum pv_act {
  PV_ACT_NONE = 0,
  PV_ACT_RELU = 1,
  PV_ACT_SWISH = 2,  /* x*sigmoid(x): pytorchvideo/layers/swish.py:7-34 */
  PV_ACT_GELU = 3,   /* exact erf form: nn.GELU default, layers/attention.py:74 */
  PV_ACT_SIGMOID = 4
};

enum pv_pool_mode { PV_POOL_MAX = 0, PV_POOL_AVG = 1 };

/* ---- library ---------------------------------------------------------------------- */
int pv_version(void);             /* ABI version, bumped on any descriptor change */
const char* pv_last_error(void);  /* text of the last PV_ERR_HIP on this thread   */
int pv_device_count(void);        /* hipGetDeviceCount; 0 when no GPU is visible  */

/* ---- dense convolution / linear as implicit GEMM on MFMA ---------------------------
 * Replaces nn.Conv3d(groups=1, dilation=1) [+ BatchNorm3d eval | + bias] [+ residual]
 * [+ activation] and nn.Linear [+ bias][+ GELU][+ residual]:
 *   models/x3d.py:169-171,210-212,297-305,480-494 (1x1x1 convs), models/resnet.py:98-132
 *   (conv_a T x1x1, conv_b 1x3x3, conv_c), models/stem.py:80-107 (stems),
 *   models/slowfast.py:672-694 (lateral 7x1x1 stride 4), models/stem.py:295-338 (patch
 *   embed), layers/attention.py:102-114,425-451,541 (Mlp / qkv / proj Linear),
 *   models/head.py:376-382 (head Linear).
 * y = act( (sum_k x'[..]*w[..]) * scale[c] + shift[c] + residual ),
 * x' = a_act(x * a_gate[b][k]) when a_gate/a_act are given (squeeze-excitation scale and
 * Swish of models/x3d.py:190-207 folded into the consumer conv_c).
 * Weights are packed [cout][kt*kh*kw][cin] (cin = padded channel count, tap-major K).
 * First-layer special case (RGB input): cin == 4 && ldx == 4 && dtype == PV_BF16 -- the input carries
 * 4 channels per voxel (8 bytes) and the weights are packed [cout][kt][kh][round_up(kw,2)][4] with
 * zeros in the padding (models/stem.py:80-107,295-338, models/x3d.py:66-88).
 */
typedef struct pv_conv3d_desc {
  const void* x;         /* input activations                                   */
  const void* w;         /* packed weights, dtype `dtype`                        */
  void* y;               /* output                                              */
  const float* scale;    /* [cout] or NULL (=1)                                 */
  const float* shift;    /* [cout] or NULL (=0)                                 */
  const void* residual;  /* same geometry as y, dtype `dtype`, or NULL           */
  const float* a_gate;   /* [B][cin] fp32 multiplier on x, or NULL               */
  int64_t x_bs, y_bs, r_bs; /* batch strides, elements                          */
  int32_t ldx, ldy, ldr;    /* voxel strides, elements                          */
  int32_t B, Ti, Hi, Wi, cin; /* cin: channels read per voxel (multiple of 8)   */
  int32_t To, Ho, Wo, cout;   /* cout: true output channels                     */
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int32_t act;           /* pv_act applied last                                  */
  int32_t a_act;         /* pv_act applied to x (after a_gate) on load           */
  int32_t dtype;         /* pv_dtype of x, w, residual                           */
  int32_t y_f32;         /* 1: y is fp32 regardless of dtype (logits, residual stream) */
  int32_t r_f32;         /* 1: residual is fp32 regardless of dtype              */
  /* Optional fused depthwise temporal conv -- the X3D stem (models/x3d.py:66-88: Conv2plus1d with
   * norm=None, activation=None between conv_xy and the depthwise 5x1x1 conv_t): when dwt_w is set
   *   y = act(scale * dwt(conv(x)) + shift),  dwt = depthwise conv over T, dwt_k taps, stride 1,
   *   padding dwt_k/2, taps [dwt_k][round_up(cout,8)] fp32.
   * Only for the first-layer layout, where pv_conv3d_dwt_supported(d) is 1. */
  const float* dwt_w;
  int32_t dwt_k;
  /* First-layer layout with at most 8 output channels (SlowFast's fast stem, models/slowfast.py:55-60):
   * c4_wpair = 2 makes two W-adjacent outputs one MFMA column, so the 16 filter rows of the matrix
   * instruction are all used and the overlapping halves of the two windows are loaded once.  Weights
   * are then packed [2][round_up(cout,8)][kt][kh][round_up(kw+sw,2)][4]: row (j, co) holds co's filter
   * shifted right by j*sw voxels, zeros elsewhere.  0 / 1 = one output per column (layout above). */
  int32_t c4_wpair;
  /* First-layer layout with an fp32 output (MViT's patch embedding, models/stem.py:289-338): the position
   * tables of SpatioTemporalClsPositionalEncoding.forward (layers/positional_encoding.py:112-136) are added
   * in the epilogue: y[to][ho][wo][c] += pos_spatial[ho*Wo+wo][c] + pos_temporal[to][c]  (separable), or
   * += pos_spatial[(to*Ho+ho)*Wo+wo][c] when pos_temporal is NULL (full table, cls row skipped by the caller).
   * Tables are fp32 [rows][cout].  The cls row itself is written by pv_add_posenc(cls_only). */
  const float* pos_spatial;
  const float* pos_temporal;
  /* Dilation of the taps (create_resnet's stage_conv_b_dilation, models/resnet.py:601-1003: the
   * detection backbone of models/hub/resnet.py:72-88 dilates res5); 0 means 1.  Dense convs only,
   * not the first-layer layout; kernel extent (k-1)*dilation+1 enters the output-size check. */
  int32_t dil_t, dil_h, dil_w;
  /* Optional second operand concatenated along K -- the projection shortcut of a residual block
   * (models/resnet.py:428-438 built, :1179-1189 added) folded into conv_c:
   *   y = act(scale * (W1 . x) + x2_scale * (W2 . x2s) + shift),  x2s[b][to][ho][wo] = x2[b][to*x2_st][ho*x2_sh][wo*x2_sw]
   * (the shortcut's strided 1x1x1 conv).  Weights [cout][round_up(cin,32) + round_up(x2_cin,32)], both parts
   * zero padded.  The two products are accumulated separately and joined in the epilogue, so the folded BatchNorm
   * scales stay fp32 exactly as in the unfused pair (shift = the two shifts added).  a_gate / a_act apply to the
   * first operand only.  Pointwise convs where pv_conv3d_x2_supported(d) is 1. */
  const void* x2;
  const float* x2_scale;     /* [cout] or NULL (=1) */
  int64_t x2_bs;
  int32_t x2_ld, x2_cin, x2_Hi, x2_Wi, x2_st, x2_sh, x2_sw;
  /* Optional pointwise conv BEHIND this conv in the same launch (round 6) -- conv_b -> conv_c of a ResNet / SlowFast
   * bottleneck (BottleneckBlock.forward, models/resnet.py:1345-1365; block built by create_bottleneck_block,
   * models/resnet.py:98-132): when pw2_w is set
   *   m = bf16(act(scale * conv(x) + shift))                       (conv_b + norm_b + act_b: `cout` channels, never stored)
   *   y = pw2_act(pw2_scale * (W2 . m) + pw2_shift + residual)     (conv_c + norm_c + the block's residual join + final act)
   * y, residual, ldy, ldr, y_bs, r_bs describe the pw2_cout-channel output; `act` is the inner activation.  W2 is
   * [pw2_cout][round_up(cout,8)] in `dtype`.  The rounding of m is the one the unfused pair has at the tensor it stores.
   * bf16 only, narrow first convs (the tap-streaming kernel's range) where pv_conv3d_pw2_supported(d) is 1. */
  const void* pw2_w;
  const float* pw2_scale;    /* [pw2_cout] or NULL (=1) */
  const float* pw2_shift;    /* [pw2_cout] or NULL (=0) */
  int32_t pw2_cout, pw2_act;
  /* The X3D stem reading the CALLER'S clip (round 7), where pv_conv3d_ncdhw_supported(d) is 1 (with dwt_w): instead of
   * pv_ingest_ncdhw copying the clip into the 4-channel layout before every forward, the stem kernel stages it from the
   * caller's NCDHW tensor itself.  x_src_slot points at 8 bytes of DEVICE memory that the kernel reads when it starts:
   *   0     -> the input is `x` in the 4-channel layout, exactly as without this field (an ingest filled it: the uint8 /
   *            normalising / frame-selecting forms of pytorchvideo_amd.transforms.DevicePacker, fp32 or strided input);
   *   other -> the address of a contiguous bf16 [B][x_src_c][Ti][Hi][Wi] tensor (any 2-byte alignment), read in place.
   * A device slot rather than a kernel argument: the captured graph (pv_plan_graph_build / pv_joint_build) keeps its
   * nodes and the way it is replayed, and follows the input through a stream-ordered 8-byte write of the slot in front
   * of the replay, made only when the address changes.  The output is bit-identical to ingest + the 4-channel stem.
   * NULL: no slot (the 4-channel layout only). */
  const void* x_src_slot;
  int32_t x_src_c;        /* channel planes of the caller's clip, 1..4 (planes beyond them read as 0) */
} pv_conv3d_desc;
int pv_conv3d(const pv_conv3d_desc* d, pv_stream_t stream);
/* 1 if this geometry (pointers are ignored) can run with the fused temporal conv, else 0 */
int pv_conv3d_dwt_supported(const pv_conv3d_desc* d);
/* 1 if this geometry (pointers are ignored; x_src_c > 0) can read the caller's NCDHW clip through x_src_slot, else 0 */
int pv_conv3d_ncdhw_supported(const pv_conv3d_desc* d);
/* 1 if this geometry (pointers are ignored; x2_cin > 0) can run with the second K operand, else 0 */
int pv_conv3d_x2_supported(const pv_conv3d_desc* d);
/* 1 if this geometry (pointers are ignored; pw2_cout > 0) can run with the pointwise conv behind it, else 0 */
int pv_conv3d_pw2_supported(const pv_conv3d_desc* d);

/* ---- development knobs ---------------------------------------------------------------------
 * Kernel-routing choices that were settled by A/B measurements on the MI355X stay overridable for the tools
 * that re-measure them (tools/bench_gemm.py, tools/gpu_*.sh): pv_tune_set("gemm8", 0) etc.  Process-wide, read
 * when an op is launched eagerly or recorded into a graph; nothing is ever read from the environment. */
int pv_tune_set(const char* key, int value);
int pv_tune_clear(void);

/* ---- SlowFast lateral connection (fast -> slow fusion) -----------------------------------
 * Replaces FuseFastToSlow.forward (models/slowfast.py:720-729) as built by
 * FastToSlowFusionBuilder.create_module (models/slowfast.py:661-694), called from
 * MultiPathWayWithFuse.forward (models/net.py:107-122):
 *   fuse = act(BatchNorm3d(Conv3d(cin -> cout, kernel (kt,1,1), stride (st,1,1), padding (pt,0,0), bias=False)(x_fast)))
 *   x_slow_fuse = torch.cat([x_slow, fuse], dim=1)
 * x is the fast pathway (B, Ti, H, W, cin) channels-last; y points at channel C_slow of the slow pathway's
 * (wider) buffer -- voxel stride ldy = that buffer's row width -- so the concatenation is the store itself.
 * Weights packed [cout][kt][cin] (cin padded to 8) in `dtype`; scale / shift = the folded BatchNorm.
 * bf16: the dedicated streaming kernel (csrc/pv_lateral.hip); fp32 parity mode: the same arithmetic through
 * pv_conv3d's (kt,1,1) path. */
typedef struct pv_lateral_desc {
  const void* x; const void* w; void* y;
  const float* scale; const float* shift;   /* [cout] or NULL */
  int64_t x_bs, y_bs;                       /* batch strides, elements */
  int32_t ldx, ldy;                         /* voxel strides, elements */
  int32_t B, Ti, H, W, cin;                 /* cin: channels read per fast voxel (multiple of 8) */
  int32_t To, cout;                         /* slow frames, true output channels */
  int32_t kt, st, pt;                       /* temporal kernel / stride (alpha) / padding */
  int32_t act, dtype;
} pv_lateral_desc;
int pv_lateral_fuse(const pv_lateral_desc* d, pv_stream_t stream);

/* ---- depthwise convolution ---------------------------------------------------------
 * Replaces nn.Conv3d(groups=C) [+ BatchNorm3d eval][+ activation]:
 *   models/x3d.py:66-88 (stem 5x1x1), models/x3d.py:180-189 (3x3x3), models/csn.py:169,
 *   layers/attention.py:363-404 (MViT pool_q/k/v; weights shared over heads -> w_mod).
 * Weights packed [taps][round_up(w_mod or C, 8)] fp32.  If psum != NULL the kernel also
 * writes per-block partial sums of the (pre-activation) output over T,H,W:
 * psum[b][blk][c], blk < pv_dwconv3d_psum_blocks(d) -- the squeeze half of
 * fvcore SqueezeExcitation (mean over T,H,W) without atomics (deterministic).
 */
typedef struct pv_dwconv3d_desc {
  const void* x; const float* w; void* y;
  const float* scale; const float* shift; /* [C] or NULL */
  float* psum;                            /* or NULL      */
  int64_t x_bs, y_bs;
  int32_t ldx, ldy;
  int32_t B, Ti, Hi, Wi, C;  /* C: true channels; round_up(C,8) are read/written */
  int32_t To, Ho, Wo;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int32_t w_mod;             /* 0, or weights indexed by (c % w_mod)             */
  int32_t act;
  int32_t dtype;
  int32_t n_prefix;          /* rows before the grid in each batch item (the cls    */
                             /* token of layers/attention.py:185-186) copied verbatim */
  /* Optional fused pointwise producer -- conv_a + norm_a + act_a of an X3D / ir-CSN bottleneck
   * (models/x3d.py:169-189, models/resnet.py:1345-1352): when pw_w is set, x is the 1x1x1 conv's
   * INPUT (pw_cin channels, row stride ldx) and the depthwise conv consumes
   * pw_act(pw_scale * (pw_w . x) + pw_shift) rounded to bf16, evaluated on the fly per halo tile --
   * the expanded tensor never exists in memory.  Only where pv_dwconv3d_pw_supported(d) is 1. */
  const void* pw_w;          /* [round_up(C,32)][round_up(pw_cin,32)] bf16, zero padded, or NULL */
  const float* pw_scale;     /* [C] or NULL */
  const float* pw_shift;     /* [C] or NULL */
  int32_t pw_cin, pw_act;
  /* Channel-wise GROUPED convolution (create_csn(stage_conv_b_width_per_group = gw), models/csn.py:34,169 ->
   * nn.Conv3d(C, C, groups = C / gw)): gw = 2, 4 or 8 input channels per output channel, all inside the output
   * channel's own 8-channel chunk.  0 / 1 = depthwise.  Weights [taps][gw][round_up(C,8)] fp32: w[t][j][c]
   * multiplies input channel (c / gw) * gw + j.  No w_mod, no fused producer, C % gw == 0. */
  int32_t gw;
} pv_dwconv3d_desc;
int pv_dwconv3d(const pv_dwconv3d_desc* d, pv_stream_t stream);
int pv_dwconv3d_psum_blocks(const pv_dwconv3d_desc* d);
/* 1 if this geometry (pointers are ignored) can run with the fused pointwise producer, else 0 */
int pv_dwconv3d_pw_supported(const pv_dwconv3d_desc* d);

/* ---- MViT attention pooling (fused) ----------------------------------------------------
 * _AttentionPool.forward with pool_mode="conv" (layers/attention.py:162-212, pools built at
 * :363-404): for up to three token tensors at once (q, k, v of one MultiScaleAttention) the
 * depthwise Conv3d over the (T,H,W) token grid (weights [taps][head_dim] fp32, shared by all
 * heads, padding = kernel/2, no bias), the cls-token pass-through (n_prefix rows) and the
 * LayerNorm(head_dim) applied to every (token, head) afterwards -- one launch instead of six.
 * Tensor i reads x[i] (B, n_prefix + Ti*Hi*Wi, heads*head_dim) with row stride ldx[i] and writes
 * y[i] (B, n_prefix + To[i]*Ho[i]*Wo[i], heads*head_dim) with row stride ldy[i].
 */
typedef struct pv_token_pool_desc {
  const void* x[3];
  void* y[3];
  const float* w[3];      /* [kt*kh*kw][head_dim]                    */
  const float* gamma[3];  /* LayerNorm weight [head_dim] or NULL     */
  const float* beta[3];   /* LayerNorm bias   [head_dim] or NULL     */
  int64_t x_bs[3], y_bs[3];
  int32_t ldx[3], ldy[3];
  int32_t st[3], sh[3], sw[3];
  int32_t To[3], Ho[3], Wo[3];
  int32_t n;              /* tensors in this launch (1..3)           */
  int32_t B, Ti, Hi, Wi, heads, head_dim;
  int32_t kt, kh, kw;
  int32_t n_prefix;
  float eps;
  int32_t dtype;
} pv_token_pool_desc;
int pv_token_pool(const pv_token_pool_desc* d, pv_stream_t stream);

/* ---- squeeze-excitation gate -------------------------------------------------------
 * fvcore.nn.squeeze_excitation.SqueezeExcitation as used at models/x3d.py:190-198:
 * gate[b][c] = sigmoid(W2 . relu(W1 . mean_{T,H,W}(x) + b1) + b2); the multiply is done
 * by the consumer (pv_conv3d a_gate).  w1 [cr][C], w2 [C][cr] fp32 row-major.
 */
typedef struct pv_se_gate_desc {
  const float* psum;   /* [B][nblk][c_p]           */
  float* gate;         /* [B][c_p]; padding = 0    */
  const float* w1; const float* b1; const float* w2; const float* b2;
  int32_t B, C, c_p, cr, nblk;
  float inv_count;     /* 1/(T*H*W)                */
} pv_se_gate_desc;
int pv_se_gate(const pv_se_gate_desc* d, pv_stream_t stream);

/* ---- pooling -----------------------------------------------------------------------
 * nn.MaxPool3d / nn.AvgPool3d (floor mode, zero/-inf padding, count_include_pad):
 *   models/stem.py:98-104 (stem max pool), models/x3d.py:791-806 and
 *   models/slowfast.py:608-620 (head average pools), layers/attention.py:677-679,720-727
 *   (MViT skip-path max pool on tokens; n_prefix = 1 copies the cls token through).
 */
typedef struct pv_pool3d_desc {
  const void* x; void* y;
  int64_t x_bs, y_bs;
  int32_t ldx, ldy;
  int32_t B, Ti, Hi, Wi, C, To, Ho, Wo;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int32_t mode;      /* pv_pool_mode */
  int32_t n_prefix;  /* rows before the grid in each batch item copied verbatim */
  int32_t dtype;
} pv_pool3d_desc;
int pv_pool3d(const pv_pool3d_desc* d, pv_stream_t stream);

/* ---- layout ingest / egress --------------------------------------------------------
 * The reference API is NCDHW (models/net.py:41-44).  Ingest converts a contiguous
 * [B,C,src_T,H,W] tensor (fp32, bf16 or uint8) to NDHWC `dtype` with C padded to c_p (zeros).
 * The steps that sit immediately before the path in the reference's data pipeline ride along
 * (SURVEY 8f-1): frame selection -- destination frame t reads source frame t_index[t], the
 * index_select of uniform_temporal_subsample (transforms/functional.py:19-41), so SlowFast's slow
 * pathway (uniform_temporal_subsample_repeated, :134-160) is ingested straight from the fast clip --
 * and a per-channel affine y = x*ch_scale[c] + ch_shift[c] in fp32, which is Div255 + Normalize
 * (transforms/transforms.py:177-195,414-430) with scale = 1/(255 std), shift = -mean/std.
 * Egress is the inverse layout change only (channels [0,C)), used by block-level forwards and tests.
 */
typedef struct pv_layout_desc {
  const void* src; void* dst;
  int32_t B, C, T, H, W;    /* logical NCDHW extent of the NCDHW side           */
  int32_t c_p, ld;          /* NDHWC side: padded channels written (multiple of 8, or 4 with ld == 4:
                               the 4-channel first-layer layout), voxel stride */
  int64_t bs;               /* NDHWC side batch stride                           */
  int32_t src_dtype, dst_dtype;
  /* ingest only (ignored by egress): */
  const int32_t* t_index;   /* [T] source frame of every destination frame, or NULL (identity)   */
  int32_t src_T;            /* frames in the source when t_index is given (else = T)              */
  const float* ch_scale;    /* [C] or NULL                                                        */
  const float* ch_shift;    /* [C] or NULL                                                        */
} pv_layout_desc;
int pv_ingest_ncdhw(const pv_layout_desc* d, pv_stream_t stream);
int pv_egress_ncdhw(const pv_layout_desc* d, pv_stream_t stream);

/* ---- short-side scale + uniform crop, fused into the ingest ---------------------------
 * What every model-zoo recipe does to a decoded frame between the frame selection and the forward:
 * short_side_scale (transforms/functional.py:92-131; module wrapper transforms/transforms.py:100-121) followed by
 * uniform_crop (functional.py:302-347; transforms.py:153-175), whose spatial_idx 0 / 1 / 2 is the three-crop test
 * protocol.  pv_resample_crop reads the decoded clip ONCE per view and writes the crop in a layout the first
 * convolution reads, with pv_layout_desc's frame selection (t_index) and Div255 + Normalize affine (ch_scale /
 * ch_shift) riding along: bilinear interpolation has weights that sum to 1, so it commutes with a per-channel affine
 * map, and the kernel interpolates the raw taps in fp32 and applies the affine map to the result.
 *
 * The geometry is computed by the caller, so the library is not tied to one scaling or cropping rule: the clip is
 * (virtually) scaled from Hs x Ws to Hn x Wn, and view v is the Ho x Wo window at (y_off[v], x_off[v]) of that.
 * The arithmetic is torch.nn.functional.interpolate(size=(Hn, Wn), mode="bilinear", align_corners=False) without
 * antialiasing, per axis in fp32:
 *     s  = (float)n_in / (float)n_out
 *     r  = max(0, s * (d + 0.5) - 0.5)          d = offset + index inside the window
 *     i0 = (int)r;  i1 = i0 + (i0 < n_in - 1);  l1 = r - i0;  l0 = 1 - l1
 *     v  = l0y (l0x p[i0y][i0x] + l1x p[i0y][i1x]) + l1y (l0x p[i1y][i0x] + l1x p[i1y][i1x])
 *     out = v * ch_scale[c] + ch_shift[c], rounded once to dst_dtype
 * Source:       PV_SRC_NCTHW  planar [B,C,src_T,Hs,Ws], PV_U8 or PV_F32 (what the decoders hand out after their permute)
 *               PV_SRC_NTHWC  frame-interleaved [B,src_T,Hs,Ws,C], PV_U8 with C == 3 (before that permute)
 * Destination:  PV_DST_NDHWC  the forms pv_ingest_ncdhw writes: c_p == 4 && ld == 4 (bf16), or c_p a multiple of 8
 *                             (bf16 / fp32); voxel stride ld, batch stride bs, pad channels written as zeros
 *               PV_DST_NCTHW  planar contiguous [n_items,C,T,Ho,Wo], bf16 / fp32 (the stem that reads the caller's clip)
 * Destination batch item b * n_views + v is view v of source clip b.  A launch writes items [item0, item0 + n_items) of
 * that sequence to positions 0 .. n_items-1 of dst (n_items == 0: all B * n_views of them), so a deploy form whose
 * batch is split over several plans is filled one plan at a time.
 * PV_ERR_INVALID: null pointers, C > 4, a window that leaves Hn x Wn, n_views outside 1..3, an interleaved source that
 * is not uint8 with C == 3, a misaligned destination.  PV_ERR_UNSUPPORTED: any other dtype / layout pair.
 */
enum pv_resample_src_layout { PV_SRC_NCTHW = 0, PV_SRC_NTHWC = 1 };
enum pv_resample_dst_layout { PV_DST_NDHWC = 0, PV_DST_NCTHW = 1 };
typedef struct pv_resample_desc {
  const void* src; void* dst;
  int32_t B, C, T;            /* source clips, channels (<= 4), DESTINATION frames                              */
  int32_t src_T, Hs, Ws;      /* source frames (used when t_index is given, else = T) and source frame size      */
  int32_t src_dtype, src_layout;
  int32_t Hn, Wn;             /* size after scaling                                                              */
  int32_t Ho, Wo;             /* crop window size                                                                */
  int32_t n_views;            /* 1..3                                                                            */
  int32_t y_off[3], x_off[3]; /* per view: the window's origin inside Hn x Wn                                    */
  int32_t item0, n_items;     /* destination items written by this launch (n_items == 0: all)                    */
  int32_t dst_layout, dst_dtype;
  int32_t c_p, ld;            /* PV_DST_NDHWC only, as in pv_layout_desc                                         */
  int64_t bs;                 /* PV_DST_NDHWC only: batch stride in elements                                     */
  const int32_t* t_index;     /* [T] source frame of every destination frame, or NULL (identity); an entry       */
                              /* outside [0, src_T-1] is clamped into it before an address is formed             */
  const float* ch_scale;      /* [C] or NULL                                                                     */
  const float* ch_shift;      /* [C] or NULL                                                                     */
} pv_resample_desc;
int pv_resample_crop(const pv_resample_desc* d, pv_stream_t stream);

/* ---- whole-video ingest: clip sampling fused into pv_resample_crop ---------------------------
 * What LabeledVideoDataset does to every video before the transforms above: a clip sampler (data/clip_sampling.py)
 * cuts it into clips, FrameVideo.get_clip (data/frame_video.py:149-200) maps each clip to a frame range and
 * UniformTemporalSubsample picks T frames of it.  All of that is a table of frame numbers, so pv_video_views reads
 * ONE decoded video through a table instead of B materialised clips through one shared index:
 * Source:       PV_SRC_NCTHW  planar [C,N,Hs,Ws], PV_U8 or PV_F32;  PV_SRC_NTHWC  [N,Hs,Ws,3], PV_U8
 * Frames:       t_index[clip * t_stride + t] (int32, device) is the video frame of destination frame t of clip `clip`;
 *               rows may overlap and repeat frames.  Every entry is CLAMPED into [0, N-1] before an address is formed,
 *               so no table can make the kernel read outside the video; reporting a bad table is the caller's job.
 * Destination item clip * n_views + v is view v of clip `clip`; item0 / n_items select ANY range of that sequence
 * (n_items == 0 with item0 == 0: all n_clips * n_views), written to positions 0 .. n_items-1 of dst.
 * Geometry, interpolation, affine map and the destination forms are pv_resample_crop's (the same kernel): a launch writes
 * bit for bit what pv_resample_crop writes for the clips materialised by index_select.
 * PV_ERR_INVALID: null src / dst / t_index, n_clips <= 0, T <= 0, N <= 0, t_stride < T, and whatever pv_resample_crop
 * rejects.  PV_ERR_UNSUPPORTED as there.
 */
typedef struct pv_video_views_desc {
  const void* src; void* dst;
  const int32_t* t_index;     /* [n_clips][t_stride], the first T of every row used                              */
  const float* ch_scale;      /* [C] or NULL                                                                     */
  const float* ch_shift;      /* [C] or NULL                                                                     */
  int64_t bs;                 /* PV_DST_NDHWC only: batch stride in elements                                     */
  int32_t n_clips, C, T;      /* table rows, channels (<= 4), DESTINATION frames per clip                        */
  int32_t N, t_stride;        /* frames in the video; table row stride (>= T)                                    */
  int32_t Hs, Ws;
  int32_t src_dtype, src_layout;
  int32_t Hn, Wn, Ho, Wo;     /* as in pv_resample_desc                                                          */
  int32_t n_views;            /* 1..3                                                                            */
  int32_t y_off[3], x_off[3];
  int32_t item0, n_items;
  int32_t dst_layout, dst_dtype;
  int32_t c_p, ld;            /* PV_DST_NDHWC only                                                               */
} pv_video_views_desc;
int pv_video_views(const pv_video_views_desc* d, pv_stream_t stream);

/* ---- decoder-native sources: YUV 4:2:0 (NV12 / NV21 / I420 / YV12) read by the ingest itself ---------------------------
 * No decoder hands out RGB: a GPU decoder writes NV12 surfaces (pitched, often with a coded height above the display
 * height), a CPU decoder planar yuv420p.  pv_yuv_views is pv_video_views on such frames: it takes the four taps of every
 * output pixel from the luma and chroma planes, converts each TAP to RGB in registers and goes on with the blend, the
 * affine map and the store above, so neither a colour-conversion pass nor an RGB copy of the video exists, and the
 * ingest reads 1.5 bytes per source pixel instead of 3.
 * Source:       N frames of uint8, frame n at src + n * frame_stride (bytes).  Inside a frame
 *                   Y(y, x) = frame[y * y_pitch + x]                                0 <= y < Hs, 0 <= x < Ws (both even)
 *                   U(j, i) = frame[u_offset + j * c_pitch + i * c_step]            0 <= j < Hs/2, 0 <= i < Ws/2
 *                   V(j, i) = frame[v_offset + j * c_pitch + i * c_step]
 *               c_step 2: one interleaved chroma plane, |v_offset - u_offset| == 1 (NV12: v_offset = u_offset + 1, NV21
 *               swapped); c_step 1: two planes (I420: U first, YV12: V first).  Rows, planes and src may start at ANY byte
 *               address: nothing needs alignment.  A coded height above Hs only moves u_offset / v_offset.
 * Frames:       t_index[clip * t_stride + t], clamped into [0, N-1] before an address is formed, as in pv_video_views.  A
 *               whole video is one such sequence; a batch of B materialised clips of T' frames is the sequence of B * T'
 *               frames with table rows b * T' + index.
 * Arithmetic:   pixel (y, x) of the VIRTUAL RGB frame is, in fp32 and NOT rounded to an integer,
 *                   rgb[c] = clamp(fma(M[c][2], V, fma(M[c][1], U, fma(M[c][0], Y, M[c][3]))), 0, 255)
 *               with Y = Y(y, x), U = U(y >> 1, x >> 1), V = V(y >> 1, x >> 1) and M = yuv2rgb, 12 fp32 values on the
 *               device: a 3 x 4 matrix, rows R, G, B, columns Y, U, V and a constant, composed by the caller -- as the
 *               caller computes the scaling geometry -- so the library is not tied to one standard or range.  Chroma is
 *               REPLICATED over its 2 x 2 luma block (the simplest well-defined rule; a filtered-chroma variant -- sited
 *               chroma, bilinear chroma upsampling -- is out of scope).  On that virtual frame the rest is exactly
 *               pv_resample_crop's formula above: the same source coordinate, the same blend order, the affine map after
 *               the blend, one rounding to dst_dtype.  The clamp sits on the taps, not behind the blend: clamping does not
 *               commute with interpolation, and "convert, then resize" is what the reference pipeline does.
 * Destination:  as pv_resample_crop (C == 3); items and item0 / n_items as pv_video_views.
 * PV_ERR_INVALID: null src / dst / t_index / yuv2rgb; n_clips, T, N <= 0; t_stride < T; odd or non-positive Hs / Ws; c_step
 * not 1 or 2; c_step 2 with |v_offset - u_offset| != 1; y_pitch < Ws; c_pitch < (Ws/2) * c_step; negative offsets; a luma or
 * chroma plane that leaves [0, frame_stride); and whatever pv_resample_crop rejects (views, windows, item range,
 * destination alignment).  PV_ERR_UNSUPPORTED: a dtype / layout pair outside pv_resample_crop's destination matrix.
 */
typedef struct pv_yuv_views_desc {
  const void* src; void* dst;
  const int32_t* t_index;     /* [n_clips][t_stride], the first T of every row used                              */
  const float* ch_scale;      /* [3] or NULL                                                                     */
  const float* ch_shift;      /* [3] or NULL                                                                     */
  const float* yuv2rgb;       /* [3][4] fp32 on the device                                                       */
  int64_t bs;                 /* PV_DST_NDHWC only: batch stride in elements                                     */
  int64_t frame_stride;       /* bytes from one frame to the next                                                */
  int64_t u_offset, v_offset; /* bytes from the start of a frame to its first U / V sample                       */
  int32_t y_pitch, c_pitch;   /* bytes per luma row (>= Ws) and per chroma row (>= (Ws/2) * c_step)              */
  int32_t c_step;             /* SAMPLES between x-adjacent samples of one chroma plane: 2 interleaved, 1 planar */
  int32_t n_clips, T;         /* table rows, DESTINATION frames per clip                                         */
  int32_t N, t_stride;        /* frames in the source; table row stride (>= T)                                   */
  int32_t Hs, Ws;             /* display size of a frame: even                                                   */
  int32_t Hn, Wn, Ho, Wo;     /* as in pv_resample_desc                                                          */
  int32_t n_views;            /* 1..3                                                                            */
  int32_t y_off[3], x_off[3];
  int32_t item0, n_items;
  int32_t dst_layout, dst_dtype;
  int32_t c_p, ld;            /* PV_DST_NDHWC only                                                               */
} pv_yuv_views_desc;
int pv_yuv_views(const pv_yuv_views_desc* d, pv_stream_t stream);

/* ---- 10- to 16-bit YUV 4:2:0 (P010 / P012 / P016, yuv420p10le and kin) read by the ingest itself ---------------------------
 * A hardware decoder given HEVC Main10, AV1 10-bit or VP9 profile 2 hands out P010: the NV12 arrangement with 16-bit
 * little-endian samples, the value in the HIGH bits; a CPU decoder hands out yuv420p10le: the I420 arrangement, the value in
 * the LOW bits.  pv_yuv16_views is pv_yuv_views on such frames -- the same descriptor, unchanged in size -- so that no
 * narrowing pass and no RGB copy stands between the decoder and the ingest.
 * Source:       N frames of 16-bit samples, frame n at src + n * frame_stride.  frame_stride, u_offset, v_offset, y_pitch and
 *               c_pitch stay in BYTES; c_step is the distance in SAMPLES (2 interleaved, 1 planar; for pv_yuv_views samples
 *               are bytes, so nothing changes there).  With s(a) the unsigned 16-bit little-endian code at byte address a,
 *                   Y(y, x) = s(frame + y * y_pitch + 2 * x)                        0 <= y < Hs, 0 <= x < Ws (both even)
 *                   U(j, i) = s(frame + u_offset + j * c_pitch + 2 * i * c_step)    0 <= j < Hs/2, 0 <= i < Ws/2
 *                   V(j, i) = s(frame + v_offset + j * c_pitch + 2 * i * c_step)
 *               c_step 2: |v_offset - u_offset| == 2 bytes (P010: v_offset = u_offset + 2; the V-first form swapped).
 *               src, frame_stride, u_offset, v_offset, y_pitch and c_pitch are EVEN: every sample lies at an even address,
 *               which is all the alignment there is (a row may start at any even byte).
 * Arithmetic:   a sample is read whole and converted exactly to fp32; it is never sign-extended, shifted or masked.  From
 *               there on the rule is pv_yuv_views' rule unchanged,
 *                   rgb[c] = clamp(fma(M[c][2], V, fma(M[c][1], U, fma(M[c][0], Y, M[c][3]))), 0, 255)
 *               per tap, chroma replicated over its 2 x 2 luma block, then pv_resample_crop's blend, affine map and single
 *               rounding to dst_dtype.  Bit depth and bit alignment are NOT the library's business: they go into M, which the
 *               caller composes, as standard and range do.  P010, P012 and P016 carry the value MSB-aligned, so their
 *               limited-range matrix is the 8-bit matrix with its Y, U, V columns scaled by 2^-8 (an exact scaling: a P016
 *               surface holding `nv12_sample << 8` gives the bits pv_yuv_views gives for the NV12 surface); an LSB-aligned
 *               10-bit stream scales them by 2^-2 around 64 / 512.  Low bits that a non-conforming decoder leaves set in an
 *               MSB-aligned sample are therefore part of the sample, worth less than one code of the stream's depth.
 * PV_ERR_INVALID: everything pv_yuv_views rejects, with row and plane extents counted at 2 bytes per sample (y_pitch < 2 Ws,
 * c_pitch < 2 (Ws/2) c_step, a last sample whose second byte leaves [0, frame_stride), c_step 2 with
 * |v_offset - u_offset| != 2); an odd src, frame_stride, u_offset, v_offset, y_pitch or c_pitch.  PV_ERR_UNSUPPORTED: as
 * pv_yuv_views; a staged strip beyond the kernels' LDS limit (two source rows of the widest window with their chroma, 64 KiB:
 * a window some 8000 columns wide).  Validation precedes every HIP call.
 * Out of scope: 4:2:2 and 4:4:4, filtered or sited chroma, big-endian samples, 16-bit RGB.  Transfer functions are not touched
 * here: the matrix is applied to the codes as they are (PQ / HLG to SDR per tap is pv_hdr_views, below).
 */
int pv_yuv16_views(const pv_yuv_views_desc* d, pv_stream_t stream);

/* ---- many videos per launch: one source per destination item ---------------------------------------------------------
 * A dataset evaluation scores thousands of videos with a handful of views each (10 clips x 3 crops, 5 x 1, 1 x 3: the model
 * zoo's test protocols), and the videos differ in length and frame size.  pv_video_views / pv_yuv_views take ONE source and
 * ONE geometry per launch, so the views of two videos cannot share a launch and a video's views rarely fill the deploy
 * batch.  pv_batch_views gives every destination item its own source: the geometry that the two entry points above take by
 * value is a RECORD per video, and an item names its record, its table row and its view.
 * Sources:      n_sources records (pv_view_source), the same bytes on the host (`sources`: the records that the launch's items
 *               name are validated, and the launch is sized from them -- a launch is usually a window of a longer sequence,
 *               and its cost does not grow with the records it does not use) and on the device (`sources_dev`: what the
 *               kernel reads).  THE CALLER UPLOADS THE VERY
 *               BUFFER IT PASSES; the library cannot compare the two, and a device copy that differs from the validated one
 *               is outside every guarantee given here.  sy / sx are (float)Hs / (float)Hn and (float)Ws / (float)Wn, divided
 *               by the caller in fp32 (the library checks the bits against its own division).
 *               src_layout PV_SRC_NCTHW: src is a dense [C,N,Hs,Ws] video, PV_U8 or PV_F32; PV_SRC_NTHWC: dense [N,Hs,Ws,3],
 *               PV_U8; PV_SRC_YUV420: N frames as in pv_yuv_views_desc (frame_stride, u_offset, v_offset, y_pitch, c_pitch).
 *               One launch has one source form: src_dtype, src_layout, C and c_step belong to the launch.  NV12 and NV21
 *               sources may share a launch (c_step 2) and so may I420 and YV12 (c_step 1): the order of U and V is the
 *               record's u_offset / v_offset.  frame_stride .. c_pitch are ignored for the RGB / planar forms.
 *               src_dtype PV_U16 with PV_SRC_YUV420: every record is a source of pv_yuv16_views (16-bit samples, byte
 *               pitches and offsets, all even, src even); item i is then bit for bit what pv_yuv16_views writes.  One launch
 *               has one sample width.  PV_U16 with an RGB / planar layout is PV_ERR_UNSUPPORTED.
 * Items:        n_items records (pv_view_item), likewise on host and device.  Item i of the launch is view items[i].view of
 *               table row items[i].row of source items[i].source and is written to position i of dst.  Any order, any mix of
 *               sources; rows and whole items may repeat.  A window of a longer sequence is a pointer offset into both
 *               copies.  The kernel clamps source / row / view into range before it uses them.
 * Frames:       ONE device table t_index[n_rows][t_stride], the rows of all videos one after another; the first T entries of
 *               a row are the video frames of the item's destination frames.  Every entry is clamped into [0, N-1] OF THE
 *               ITEM'S SOURCE before an address is formed; reporting a bad table is the caller's job.
 * Arithmetic:   pv_resample_crop's pinned formula and, for PV_SRC_YUV420, pv_yuv_views' rule, tap clamp included.  Item i is
 *               bit for bit what pv_video_views / pv_yuv_views writes for that video alone with
 *               item0 = row * n_views + view, n_items = 1.
 * Destination:  the forms, strides and alignment of pv_resample_crop; ch_scale / ch_shift as there.
 * PV_ERR_INVALID: null sources / sources_dev / items / items_dev / t_index / dst (yuv2rgb for PV_SRC_YUV420); n_sources,
 * n_items, n_rows, T, C, Ho, Wo <= 0; t_stride < T; n_items or T > 65535 (the grid); an item whose source, row or view is out
 * of range; a record named by an item with a null src, non-positive N / Hs / Ws / Hn / Wn, a view window that leaves Hn x Wn,
 * sy / sx whose bits are not the library's own division, or -- PV_F32 sources -- a src that is no multiple of 4; whatever pv_resample_crop rejects (C > 4, an interleaved source that is not uint8 with C == 3,
 * destination alignment, n_views outside 1..3); for PV_SRC_YUV420, per such record, the plane checks of pv_yuv_views (odd sizes,
 * pitches, offsets, planes inside frame_stride) and C != 3.  PV_ERR_UNSUPPORTED: the dtype / layout matrix of
 * pv_resample_crop, and a staged strip beyond the kernels' LDS limit.
 * Orientation:  a phone video recorded upright is STORED as landscape frames plus a display matrix ("rotate 90"), a front
 *               camera adds a mirror, and a decoder hands out the stored frames.  pv_view_source.orient (the field that used
 *               to be `reserved`: same offset and size, 0 in every record built before) = rot | (mirror << 2), rot 0..3,
 *               mirror 0 / 1.  Hs, Ws, pitches, offsets and frame_stride keep describing the STORED frame S -- addresses
 *               depend on them.  The DISPLAYED frame D is Hd x Wd = (rot & 1) ? Ws x Hs : Hs x Ws and, with
 *               x' = mirror ? Wd-1-x : x,
 *                   rot 0: D(y,x) = S(y, x')             the stored frame as it lies
 *                   rot 1: D(y,x) = S(Hs-1-x', y)        turned 90 degrees clockwise: a decoder's "rotation 90"
 *                   rot 2: D(y,x) = S(Hs-1-y, Ws-1-x')   turned 180 degrees
 *                   rot 3: D(y,x) = S(x', Ws-1-y)        turned 270 degrees clockwise
 *               -- torch.rot90(S, -rot, (h, w)), then .flip(w) if mirror.  Everything downstream is defined ON D: Hn, Wn
 *               and the view windows are displayed coordinates, sy = (float)Hd / (float)Hn and sx = (float)Wd / (float)Wn
 *               (the bit check uses these); the pinned coordinate, the blend order, the tap clamp of YUV, the affine map
 *               and the single rounding are unchanged.  For YUV 4:2:0 the chroma of displayed pixel (y,x) is the chroma
 *               sample of the stored pixel it maps to; Hs and Ws are even, so that is the Y, U and V planes oriented
 *               separately.  Hence: AN ITEM OF AN ORIENTED RECORD HOLDS, BIT FOR BIT, WHAT THE SAME LAUNCH WRITES FOR A
 *               DENSE COPY OF THE VIDEO THAT WAS ORIENTED BEFOREHAND, WITH orient = 0.  Honoured by pv_batch_views and
 *               pv_frame_views in every source form, and by pv_box_views; one launch may mix orientations freely.  Items
 *               of upright records run the staged-strip kernels exactly as before; items of oriented records run a tile
 *               kernel (a workgroup stages the stored footprint of a tile of displayed rows x columns), each maximal run
 *               of items of one kind as one kernel launch.  The one-source entry points (pv_resample_crop, pv_video_views,
 *               pv_yuv_views, pv_yuv16_views) have no field for it.  PV_ERR_INVALID: orient outside 0..7; sy / sx whose
 *               bits are not the displayed-size quotient; a window that leaves Hn x Wn.  PV_ERR_UNSUPPORTED: a staged
 *               tile footprint beyond the LDS limit.
 */
enum { PV_SRC_YUV420 = 2 };   /* pv_batch_views_desc.src_layout only, beside pv_resample_src_layout */
/* Packed pixels (see "packed pixels" below); pv_batch_views_desc.src_layout only.  The value 3 is no layout. */
enum { PV_SRC_BGR = 4, PV_SRC_RGBA = 5, PV_SRC_BGRA = 6, PV_SRC_ARGB = 7, PV_SRC_ABGR = 8 };
/* YUV 4:2:2 and 4:4:4 (see "YUV 4:2:2 and 4:4:4" below); pv_batch_views_desc.src_layout only.  The value 9 is no layout. */
enum { PV_SRC_YUV422 = 10, PV_SRC_YUV444 = 11 };
/* Packed YUV 4:2:2 (see "packed YUV 4:2:2" below); pv_batch_views_desc.src_layout only.  The value 12 is no layout. */
enum { PV_SRC_YUYV422 = 13 };
typedef struct pv_view_source {      /* one decoded video; 96 bytes, 8-byte aligned */
  const void* src;                   /* device address of the video / of frame 0                              */
  int64_t frame_stride;              /* YUV and packed sources: bytes between frames (RGB / planar: dense)    */
  int64_t u_offset, v_offset;        /* YUV sources, as in pv_yuv_views_desc                                   */
  int32_t y_pitch, c_pitch;          /* YUV sources; packed pixels: y_pitch = the row pitch, c_pitch = 0      */
  int32_t N, Hs, Ws;                 /* frames, frame size                                                     */
  int32_t Hn, Wn;                    /* size after scaling                                                     */
  int32_t y_off[3], x_off[3];        /* per view: window origin inside Hn x Wn                                 */
  float   sy, sx;                    /* (float)Hd / (float)Hn, (float)Wd / (float)Wn of the DISPLAYED frame    */
  int32_t orient;                    /* rot | (mirror << 2): see "orientation" above; 0 = the stored frame    */
} pv_view_source;
typedef struct pv_view_item { int32_t source, row, view, reserved; } pv_view_item;   /* one destination item */
typedef struct pv_batch_views_desc {
  const pv_view_source* sources;      /* [n_sources] on the HOST                                               */
  const pv_view_source* sources_dev;  /* the same bytes on the device                                          */
  const pv_view_item* items;          /* [n_items] on the HOST                                                 */
  const pv_view_item* items_dev;      /* the same bytes on the device                                          */
  const int32_t* t_index;             /* [n_rows][t_stride] on the device, the first T of every row used       */
  void* dst;
  const float* ch_scale;              /* [C] or NULL                                                           */
  const float* ch_shift;              /* [C] or NULL                                                           */
  const float* yuv2rgb;               /* PV_SRC_YUV420 / 422 / 444: [3][4] fp32 on the device                  */
  int64_t bs;                         /* PV_DST_NDHWC only: batch stride in elements                           */
  int32_t n_sources, n_items, n_rows, t_stride;
  int32_t C, T;                       /* channels (<= 4; 3 for YUV), DESTINATION frames per item               */
  int32_t src_dtype, src_layout;      /* pv_dtype; PV_SRC_NCTHW / PV_SRC_NTHWC / PV_SRC_YUV420 / PV_SRC_BGR .. */
  int32_t c_step;                     /* PV_SRC_YUV420 / 422 / 444: 2 interleaved chroma, 1 planar; YUYV422: 4 */
  int32_t Ho, Wo, n_views;            /* crop window; views per clip, 1..3                                     */
  int32_t dst_layout, dst_dtype;
  int32_t c_p, ld;                    /* PV_DST_NDHWC only                                                     */
} pv_batch_views_desc;
int pv_batch_views(const pv_batch_views_desc* d, pv_stream_t stream);

/* ---- frame-list sources: every frame individually addressed ------------------------------------------------------------
 * pv_batch_views reads a video as ONE allocation with a constant frame stride.  A hardware decoder hands out surfaces from a
 * pool -- one allocation per frame, uniform geometry and pitch, any order, reused -- and a live stream never is one tensor.
 * pv_frame_views is pv_batch_views with a source given as a list of frame addresses: nothing is copied together first.
 * Launch:       `batch`, a whole pv_batch_views_desc with the meaning it has there, except sources[i].src.
 * Frames:       ONE table frame_ptrs[n_frame_ptrs] of 64-bit device addresses for the launch, on the host (`frame_ptrs`:
 *               validated) and the same bytes on the device (`frame_ptrs_dev`: what the kernel reads), under the rule of
 *               sources / sources_dev: THE CALLER UPLOADS THE VERY BUFFER IT PASSES.  The `src` of a record is the DEVICE
 *               address of the record's slice of the table, frame_ptrs_dev + k (8-byte aligned); the slice's N entries are the
 *               base addresses of frames 0 .. N-1.  An address may appear any number of times, in any slice.  The record
 *               keeps its 96 bytes and pv_box_views reads the same records (it never follows `src`).
 * One frame:    PV_SRC_NTHWC: dense [Hs,Ws,3], PV_U8.  PV_SRC_NCTHW: dense [C,Hs,Ws] -- the plane stride is that of ONE
 *               frame --, PV_U8 or PV_F32.  PV_SRC_YUV420: one surface as in pv_yuv_views_desc (u_offset, v_offset, y_pitch,
 *               c_pitch from the frame's base); frame_stride keeps its meaning as the extent of one frame, for the plane
 *               checks.  uint8 frames may start at any byte; fp32 frames at a multiple of 4; the frames of a PV_U16
 *               launch (PV_SRC_YUV420 only, as in pv_batch_views) at an even address, read from the host copy.  One launch
 *               has one form.
 * Table entry:  clamped into [0, N-1] OF THE ITEM'S SOURCE before the slice is indexed, as pv_batch_views clamps it before
 *               the multiply.  Only the aligned 16-byte granules that cover a byte of a staged span are fetched, so a frame
 *               that ends at the end of its allocation is read safely.
 * Arithmetic:   item i is bit for bit what pv_batch_views writes for the same frames laid out as one video.
 * PV_ERR_INVALID: whatever pv_batch_views rejects; a null frame_ptrs or frame_ptrs_dev, a frame_ptrs_dev that is no multiple
 * of 8, n_frame_ptrs <= 0; a record named by an item whose src is not frame_ptrs_dev + 8 k with 0 <= k and
 * k + N <= n_frame_ptrs; a null frame address in such a slice (read from the host copy); PV_F32 sources with a frame address
 * that is no multiple of 4.  PV_ERR_UNSUPPORTED: as pv_batch_views.  Validation precedes every HIP call.
 */
typedef struct pv_frame_views_desc {
  pv_batch_views_desc batch;          /* as for pv_batch_views; sources[i].src = frame_ptrs_dev + first_i       */
  const uint64_t* frame_ptrs;         /* [n_frame_ptrs] on the HOST: device addresses of frames                */
  const uint64_t* frame_ptrs_dev;     /* the same bytes on the device                                          */
  int32_t n_frame_ptrs;
  int32_t reserved;
} pv_frame_views_desc;
int pv_frame_views(const pv_frame_views_desc* d, pv_stream_t stream);

/* ---- HDR sources: PQ / HLG taps converted to BT.709 SDR inside the launch ------------------------------------------------
 * Most 10-bit streams are HDR: a phone's HLG (BT.2100, usually stored rotated), HDR10 / AV1 PQ (SMPTE ST 2084).  Their
 * samples give BT.2020 R'G'B' under a PQ or HLG curve, and a network trained on BT.709 SDR reads mid-greys tens of codes off
 * and the wrong primaries.  pv_hdr_views is pv_batch_views / pv_frame_views on 16-bit YUV 4:2:0 sources with one more step
 * PER TAP, in registers: no colour pass over the video and no RGB copy stands between the decoder and the ingest.
 * Launch:       `frames`, a whole pv_frame_views_desc.  frames.frame_ptrs == NULL (and frame_ptrs_dev NULL, n_frame_ptrs 0):
 *               the records are whole videos, exactly pv_batch_views' meaning of frames.batch; otherwise pv_frame_views'
 *               meaning.  src_layout PV_SRC_YUV420 with src_dtype PV_U16 only.  pv_view_source.orient is honoured and a
 *               launch may mix orientations, as there.
 * Arithmetic:   the rule of pv_yuv_views stands: convert each tap, then blend.  A tap of the virtual RGB frame is
 *               rgb[c] = clamp(M (Y,U,V,1), 0, 255) as in pv_yuv16_views, M the caller's matrix (BT.2020, the stream's depth and
 *               bit alignment).  With e_c = rgb[c] / 255 every tap is then mapped in fp32, tone[16] being fp32 values the
 *               caller composes (transforms.tone_params) and uploads:
 *                 1. to linear light in units of SDR reference white.
 *                    PV_TRANSFER_PQ:  p = e^(1/m2), l_c = (max(p - c1, 0) / (c2 - c3 p))^(1/m1) * tone[0], with m1 = 2610/16384,
 *                    m2 = 2523/4096 * 128, c1 = 3424/4096, c2 = 2413/4096 * 32, c3 = 2392/4096 * 32; tone[0] = 10000 / white_nits.
 *                    PV_TRANSFER_HLG: s_c = e^2 / 3 for e <= 1/2, else (exp((e - c) / a) + b) / 12, a = 0.17883277, b = 1 - 4a,
 *                    c = 0.5 - a ln(4a); Ys = 0.2627 s_R + 0.6780 s_G + 0.0593 s_B; l_c = s_c * Ys^tone[1] * tone[0], with
 *                    tone[1] = gamma - 1 and tone[0] = peak_nits / white_nits.  No black-level lift; Ys = 0 gives 0.
 *                 2. tone curve on max-RGB, hue-preserving ("mobius"): m = max(l_R, l_G, l_B),
 *                    k = m > j ? s (m + a') / ((m + b') m) : 1, l_c *= k, with j, s, a', b' = tone[2..5].  j = 3e38 disables
 *                    the curve (step 3 then clips).
 *                 3. gamut: l = clamp(G l, 0, 1), G = tone[6..14] row-major (BT.2020 to BT.709, or the identity).
 *                 4. back to a BT.709-coded signal with BT.2020's continuous constants: v = 4.5 l for l < 0.018053968510807,
 *                    else 1.09929682680944 l^0.45 - 0.09929682680944.  The tap becomes 255 v.
 *               tone[15] is 0.  x^y is exp2(y log2 x) on the hardware's transcendental units (1 ulp each), divisions are
 *               multiplications by the hardware reciprocal; a zero base gives 0, never NaN: all-zero and all-0xFFFF surfaces
 *               give finite output.  From there on: pv_resample_crop's blend, affine map and single rounding, unchanged.
 *               Item i holds the same bits whatever else shares its launch, for a frame list as for the stacked video, and
 *               for an oriented record as for a copy oriented beforehand.
 * PV_ERR_INVALID: a null descriptor or tone; transfer outside 1..2; reserved != 0; a pointer table only half given
 * (frame_ptrs without frame_ptrs_dev or the reverse), or n_frame_ptrs != 0 without a table; whatever the wrapped entry point
 * rejects.  PV_ERR_UNSUPPORTED: any src_layout / src_dtype pair but PV_SRC_YUV420 / PV_U16 (8-bit HDR does not exist in
 * practice); as the wrapped entry point otherwise.  Validation precedes every HIP call.
 * Out of scope: dynamic metadata (HDR10+, Dolby Vision), BT.2390 / scene-adaptive curves, a transfer per record.
 */
enum { PV_TRANSFER_PQ = 1, PV_TRANSFER_HLG = 2 };
typedef struct pv_hdr_views_desc {
  pv_frame_views_desc frames;         /* frame_ptrs == NULL: whole videos (pv_batch_views); else pv_frame_views  */
  const float* tone;                  /* [16] fp32 on the device, see "arithmetic"                              */
  int32_t transfer;                   /* PV_TRANSFER_PQ / PV_TRANSFER_HLG                                       */
  int32_t reserved;                   /* 0                                                                      */
} pv_hdr_views_desc;                  /* sizeof(pv_frame_views_desc) + 16 */
int pv_hdr_views(const pv_hdr_views_desc* d, pv_stream_t stream);

/* ---- a rectangle per frame: actor tubes resized in place ---------------------------------------------------------------------
 * A detector and a tracker find people, and a classifier is run on each of them: a rectangle of the frame, of any size and
 * aspect and usually moving from frame to frame, is cut out and resized to the network's input (the deterministic core of the
 * reference's random_resized_crop: crop, then interpolate(size=(Ho, Wo), mode="bilinear")).  pv_batch_views cannot say that:
 * its scale is Hd / Hn with an integer Hn, and it has one geometry per video.  pv_region_views is pv_batch_views /
 * pv_frame_views with the geometry taken from a 32-byte record PER DESTINATION FRAME of every table row; the video is read where
 * it lies, once, and no crop, no RGB copy of a YUV source and no resized tube is materialised.
 * Launch:       `frames`, a whole pv_frame_views_desc.  frames.frame_ptrs == NULL (and frame_ptrs_dev NULL, n_frame_ptrs 0):
 *               the records are whole videos, pv_batch_views' meaning of frames.batch; otherwise pv_frame_views' meaning.
 *               n_views == 1 and every item's view == 0.  Item i is (source, row, view) as there.
 * Regions:      regions[n_rows][t_stride], indexed exactly like t_index, on the host (`regions`: validated, and the launch is
 *               sized from it) and the same bytes on the device (`regions_dev`, a multiple of 4: what the kernel reads), under
 *               the rule of sources / sources_dev.  For destination frame t of an item the frame is t_index[row][t], clamped as
 *               in pv_batch_views, and the rectangle is regions[row][t]: rows [top, top + h) x columns [left, left + w) of it.
 *               sy = (float)h / (float)Ho and sx = (float)w / (float)Wo, divided by the caller in fp32.
 * Arithmetic:   the output frame is the Ho x Wo bilinear resize of that rectangle ALONE: per axis pv_resample_crop's pinned
 *               coordinate with s = sy, d = 0 .. Ho-1 and n_in = h, so that no tap leaves the rectangle -- crop, then
 *               interpolate, not a window of the scaled full frame.  The source row of a tap is top + i0 / top + i1, columns
 *               likewise.  Blend order, the YUV tap rule (every tap converted and clamped; the chroma of the ABSOLUTE pixel),
 *               the affine map and the single rounding are unchanged.  Of a record, Hn, Wn, y_off, x_off, sy and sx are NOT
 *               read.  ITEM i, FRAME t HOLDS, BIT FOR BIT, WHAT pv_batch_views WRITES FOR A DENSE ONE-FRAME COPY OF THAT
 *               RECTANGLE GIVEN AS A SOURCE OF ITS OWN, with Hn = Ho, Wn = Wo and offsets 0 -- whatever else shares the launch,
 *               and for a frame list as for the stacked video.
 * Source forms: the upright forms of pv_batch_views / pv_frame_views: PV_SRC_NTHWC PV_U8, PV_SRC_NCTHW PV_U8 / PV_F32,
 *               PV_SRC_YUV420 PV_U8 / PV_U16 with either c_step.  For PV_SRC_YUV420 top, left, h and w are all even: a dense
 *               4:2:0 copy of the rectangle then exists, which is what the guarantee above is stated against.
 * The kernel clamps top / left / h / w into the item's source frame before it forms an address: a device copy that differs from
 * the validated one cannot read outside the video.
 * PV_ERR_INVALID: a null descriptor, regions or regions_dev, a regions_dev that is no multiple of 4; a pointer table only half
 * given, or n_frame_ptrs != 0 without a table; n_views != 1 or an item with view != 0; for every item of the launch and every
 * t < T a rectangle with h < 1 or w < 1, one that leaves [0, Hs) x [0, Ws) of the item's source, sy / sx whose bits are not the
 * library's own division, a non-zero reserved, or -- PV_SRC_YUV420 -- an odd member; whatever the wrapped entry point rejects
 * (but nothing about the record fields named above).  PV_ERR_UNSUPPORTED: a record named by an item with orient != 0; a
 * staged strip beyond the kernels' LDS limit; as the wrapped entry point otherwise.  Validation precedes every HIP call.
 * Out of scope: oriented records (orient != 0) and the PQ / HLG tap map of pv_hdr_views.
 */
typedef struct pv_view_region {      /* 32 bytes: one rectangle of the frame, for ONE destination frame of ONE table row */
  int32_t top, left, h, w;           /* rows [top, top+h) x columns [left, left+w) of the source frame                  */
  float   sy, sx;                    /* (float)h / (float)Ho, (float)w / (float)Wo, divided by the caller in fp32        */
  int32_t reserved[2];               /* 0                                                                                */
} pv_view_region;
typedef struct pv_region_views_desc {
  pv_frame_views_desc frames;         /* frame_ptrs == NULL: whole videos (pv_batch_views' meaning); else pv_frame_views' */
  const pv_view_region* regions;      /* [n_rows][t_stride] on the HOST, indexed exactly like t_index                     */
  const pv_view_region* regions_dev;  /* the same bytes on the device                                                     */
} pv_region_views_desc;               /* sizeof(pv_frame_views_desc) + 16 */
int pv_region_views(const pv_region_views_desc* d, pv_stream_t stream);

/* ---- box-filtered downscale: interpolation="area" inside the launch ---------------------------------------------------------
 * pv_resample_crop's four taps per output pixel are right for sources that were shrunk beforehand.  A decoder surface of 1080p
 * scaled to a short side of 256 has some 18 source pixels under every output pixel (2160p: 70), and four taps of them are point
 * sampling: aliasing, moire, noise at full amplitude.  The reference's downscale mode for that is interpolation="area"
 * (short_side_scale / ShortSideScale / short_side_scale_with_boxes pass it to F.interpolate; transforms/functional.py:92-131,
 * 195-231): adaptive average pooling, a box filter.  pv_area_views is pv_batch_views / pv_frame_views with that filter in place
 * of the blend; the video is read where it lies, and no float RGB copy, interpolate pass or crop is materialised.
 * Launch:       `frames`, a whole pv_frame_views_desc.  frames.frame_ptrs == NULL (and frame_ptrs_dev NULL, n_frame_ptrs 0):
 *               the records are whole videos, pv_batch_views' meaning of frames.batch; otherwise pv_frame_views' meaning.
 *               Records, items, the frame table, views, destination forms, the affine map and the item window are the wrapped
 *               entry point's; the same pv_view_source records serve both filters: sy / sx are validated as there (their bits
 *               against the library's own division) and NOT used by the arithmetic.  filter = PV_FILTER_AREA.
 * Arithmetic:   per axis, for destination index d of the virtually scaled frame (d = window offset + index inside the window,
 *               n_in = Hs or Ws, n_out = Hn or Wn), in integers with floor division:
 *                   start = (d * n_in) / n_out;   end = ((d + 1) * n_in + n_out - 1) / n_out          (end > start always)
 *               The value is the mean of the taps in rows [start_y, end_y) x columns [start_x, end_x): exactly the windows of
 *               torch.nn.functional.interpolate(size=(Hn, Wn), mode="area").  Windows of neighbouring outputs overlap by one
 *               row or column when the ratio is no integer; upscaling gives windows of one or two pixels.  The order is pinned,
 *               so that every instantiation gives the same bits: per channel
 *                   1. for each source column of the window, the fp32 sum of its taps over the window's rows, ascending;
 *                   2. the fp32 sum of those column sums over the window's columns, ascending;
 *                   3. ONE IEEE division by (float)((end_y - start_y) * (end_x - start_x));
 *                   4. out = fmaf(v, ch_scale[c], ch_shift[c]), rounded once to dst_dtype.
 *               For uint8 RGB / planar sources the sums are exact integers.  PV_SRC_YUV420 (8- and 16-bit): pv_yuv_views' rule
 *               stands -- every tap is converted and clamped first, rgb[c] = clamp(M (Y,U,V,1), 0, 255) with the chroma of
 *               pixel (y, x) the sample at (y >> 1, x >> 1), THEN averaged; the clamp makes averaging Y, U and V separately a
 *               different function.
 *               Item i holds the same bits whatever else shares its launch (strip height, column tile and LDS pitch are sized
 *               from the launch's widest record and enter no value), and the same bits for a frame list as for the stacked
 *               video.  Where Hn == Hs and Wn == Ws every window is one pixel and item i holds, bit for bit, what pv_batch_views
 *               writes (whose weights are then 1 and 0).
 * Index limit:  Hs * Hn <= 2^24 and Ws * Wn <= 2^24 for every record an item names.  Beyond it torch's own index arithmetic is
 *               done in float and is no longer the integer one above, so no reference would exist.
 * Source forms: the upright forms of pv_batch_views / pv_frame_views: PV_SRC_NTHWC PV_U8, PV_SRC_NCTHW PV_U8 / PV_F32,
 *               PV_SRC_YUV420 PV_U8 / PV_U16 with either c_step, pitched surfaces, coded heights, any byte base as there.
 * PV_ERR_INVALID: a null descriptor; filter outside {PV_FILTER_AREA}; a non-zero reserved; a pointer table only half given, or
 * n_frame_ptrs != 0 without a table; whatever the wrapped entry point rejects.  PV_ERR_UNSUPPORTED: a record named by an item
 * with orient != 0; the index limit; the dtype / layout matrix of the wrapped entry point; a window so large that the source
 * rectangle under ONE output row x 8 output columns, in the source dtype, exceeds the kernels' LDS limit of 64 KiB (some 2000
 * taps per channel plane: a ratio beyond 50 for uint8 sources and 25 for fp32 ones; the frame WIDTH is no limit, a workgroup
 * owns a tile of columns).  Validation precedes every HIP call.
 * Out of scope: oriented records (orient != 0), the PQ / HLG tap map of pv_hdr_views, pv_region_views' rectangles (tubes are
 * resized by about 1-2x), the one-source entry points, bicubic and nearest.
 */
enum { PV_FILTER_AREA = 1 };
typedef struct pv_area_views_desc {
  pv_frame_views_desc frames;         /* frame_ptrs == NULL: whole videos (pv_batch_views' meaning); else pv_frame_views' */
  int32_t filter;                     /* PV_FILTER_AREA                                                                   */
  int32_t reserved[3];                /* 0                                                                                */
} pv_area_views_desc;                 /* sizeof(pv_frame_views_desc) + 16 */
int pv_area_views(const pv_area_views_desc* d, pv_stream_t stream);

/* ---- packed pixels: BGR24 and 32-bit RGBA / BGRA / ARGB / ABGR surfaces read where they lie ---------------------------------
 * An OpenCV pipeline holds BGR24; screen capture, colour converters, compositor / DRM / GL surfaces and `-pix_fmt bgra|rgb0`
 * hand out 32-bit pixels, usually PITCHED.  PV_SRC_NTHWC is dense R,G,B only, so such frames needed a channel-select pass plus
 * copy over the whole video before the launch.  Five more values of pv_batch_views_desc.src_layout (declared beside
 * PV_SRC_YUV420; the value 3 is no layout and stays PV_ERR_INVALID) name them:
 *                   PV_SRC_BGR   3 bytes a pixel: B G R           PV_SRC_RGBA  4 bytes: R G B x       PV_SRC_BGRA  4 bytes: B G R x
 *                   PV_SRC_ARGB  4 bytes: x R G B                 PV_SRC_ABGR  4 bytes: x B G R
 *               The layout alone gives the pixel size PB (3 or 4) and the bytes of R, G and B inside a pixel; x (alpha, or
 *               the unused byte of RGBX / BGRX / XRGB / XBGR) never enters a value.
 * Honoured by:  pv_batch_views, pv_frame_views, pv_region_views and pv_area_views -- whole videos and frame lists, orient 0..7
 *               where the entry point takes it, up to three views, all five destination forms.  NOT by pv_hdr_views (16-bit
 *               YUV only) and not by the one-source entry points (pv_resample_crop, pv_video_views, pv_yuv_views,
 *               pv_yuv16_views): their refusals are what they were.
 * Record:       src_dtype PV_U8 and C == 3 (the launch); per pv_view_source
 *                   pixel(y, x) = frame + y * y_pitch + x * PB                        0 <= y < Hs, 0 <= x < Ws
 *               y_pitch: the ROW PITCH IN BYTES, >= Ws * PB.  frame_stride: the bytes between frames (whole videos) or the
 *               extent of one frame (frame lists), >= (Hs - 1) * y_pitch + Ws * PB.  u_offset, v_offset and c_pitch are 0.
 *               PB == 4: src -- or every frame address of a list --, y_pitch and frame_stride are multiples of 4: a pixel is
 *               one aligned dword.  PB == 3: any byte base, any pitch.  A column slice of a wider surface is a record whose
 *               src points at the slice's first pixel and whose y_pitch is the surface's.
 *               Only the aligned 16-byte granules that cover a byte of a staged span are fetched, as for every other source,
 *               so a surface that ends at the end of its allocation is read safely; the bytes between Ws * PB and the pitch
 *               are never read from the staged rows.
 * Arithmetic:   nothing new happens to a value: the taps, the pinned coordinate, the blend order, the windows and the
 *               summation order of pv_area_views, the rectangles of pv_region_views, the affine map and the single rounding are
 *               those of the PV_SRC_NTHWC path.  AN ITEM OF A PACKED LAUNCH HOLDS, BIT FOR BIT, WHAT THE SAME ENTRY POINT WRITES
 *               WITH PV_SRC_NTHWC FOR THE DENSE [N,Hs,Ws,3] R,G,B COPY OF THE SAME FRAMES -- whatever else shares the launch,
 *               and for a frame list as for the stacked video.
 * Kernels:      pixel size is compiled in (two source forms), the three byte offsets are a workgroup-uniform kernel argument;
 *               a 4-byte pixel is one dword LDS read per tap with the channels taken out of the register, a 3-byte pixel
 *               three byte reads (pytorchvideo_amd/csrc/pv_packed.hip).
 * PV_ERR_INVALID: y_pitch < Ws * PB; frame_stride < (Hs - 1) * y_pitch + Ws * PB; a non-zero u_offset, v_offset or c_pitch;
 * src_dtype != PV_U8 or C != 3; PB == 4 with a src, frame address, y_pitch or frame_stride that is no multiple of 4; and
 * whatever the entry point rejects of any launch.  PV_ERR_UNSUPPORTED: unchanged in meaning (the LDS limits of a staged strip
 * or tile -- a column counts PB bytes --, the index limit of pv_area_views, src_dtype PV_U16 outside YUV).  Validation precedes
 * every HIP call, and an invalid field wins over an unsupported size.
 */

/* ---- YUV 4:2:2 and 4:4:4: planar and semi-planar frames of 8- to 16-bit samples read where they lie -----------------------
 * A CPU decoder hands out more than 4:2:0: yuvj422p from MJPEG (most USB and IP cameras), yuv422p10le from ProRes / DNxHR and
 * contribution feeds, NV16 / P210 from capture SDKs, yuv444p / yuv444p10le from screen recordings, High 4:4:4 streams and
 * lossless archives.  PV_SRC_YUV420 hard-wires the chroma of pixel (y, x) to (y >> 1, x >> 1), so such a video needed a chroma
 * decimation into a 4:2:0 copy, or an RGB copy, before the launch.  Two more values of pv_batch_views_desc.src_layout (declared
 * beside PV_SRC_YUV420; the value 9 is no layout and stays PV_ERR_INVALID) name them:
 *                   PV_SRC_YUV422   (csy, csx) = (0, 1): chroma halved in x only        PV_SRC_YUV444   (0, 0): full-size chroma
 *               (PV_SRC_YUV420 is (1, 1)).  The subsampling belongs to the LAUNCH, as c_step and the sample width do.
 * Honoured by:  pv_batch_views, pv_frame_views, pv_region_views and pv_area_views -- whole videos and frame lists, orient 0..7
 *               where the entry point takes it, up to three views, all five destination forms.  NOT by pv_hdr_views, which
 *               answers PV_ERR_UNSUPPORTED as for everything but 16-bit 4:2:0, and not by the one-source entry points
 *               (pv_resample_crop, pv_video_views, pv_yuv_views, pv_yuv16_views), which have no field for them.
 * Record:       the fields of a PV_SRC_YUV420 record with the same meaning, in bytes; sb = 1 (PV_U8) or 2 (PV_U16):
 *                   Y(y, x) = frame[y * y_pitch + x * sb]                                  0 <= y < Hs, 0 <= x < Ws
 *                   U(j, i) = frame[u_offset + j * c_pitch + i * c_step * sb]              0 <= j < ceil(Hs / 2^csy),
 *                   V(j, i) = frame[v_offset + j * c_pitch + i * c_step * sb]              0 <= i < ceil(Ws / 2^csx)
 *                   tap (y, x) uses U(y >> csy, x >> csx) and V(y >> csy, x >> csx)
 *               c_step 1 (two planes: yuv422p, yuv444p and their 10- to 16-bit kin) and c_step 2 (one interleaved plane,
 *               |v_offset - u_offset| == sb: NV16 / NV61 / P210, and with PV_SRC_YUV444 NV24 / NV42) are valid with both.
 *               PV_SRC_YUV422 needs an even Ws and takes any Hs; PV_SRC_YUV444 takes any Hs and Ws, odd included.  PV_U16: the
 *               evenness rules of pv_yuv16_views (src or every frame address, pitches, offsets and frame_stride even).  Pitched
 *               surfaces and coded heights are what y_pitch, c_pitch and the offsets say; depth and bit alignment live in
 *               yuv2rgb, as for P010 / yuv420p10le.
 * pv_region_views: only the members the subsampling halves are even: left and w for PV_SRC_YUV422, none for PV_SRC_YUV444.
 * Arithmetic:   pv_yuv_views' pinned rule, unchanged: each tap is converted with the three fused multiply-adds and clamped, then
 *               the pinned blend or the pinned window sums of pv_area_views, the affine map, one rounding.  Chroma is REPLICATED
 *               over the luma pixels it covers; sited or filtered chroma stays out of scope.  Hence the guarantee of every new
 *               launch: AN ITEM HOLDS, BIT FOR BIT, WHAT THE SAME ENTRY POINT WRITES WITH PV_SRC_YUV444 FOR THE FRAMES WHOSE
 *               CHROMA PLANES HOLD EVERY SAMPLE REPLICATED OVER THE PIXELS IT COVERS -- and a PV_SRC_YUV420 launch holds what
 *               both new layouts write for its replicated copies.
 * Orientation:  for a subsampled layout a quarter turn of the STORED frame is no layout of its own (4:2:2 turned is chroma halved
 *               in y), so the contract of an oriented record is stated through the full-resolution copy: the chroma of displayed
 *               pixel (y, x) is the chroma sample of the stored pixel it maps to, and AN ITEM OF AN ORIENTED RECORD HOLDS, BIT
 *               FOR BIT, WHAT THE SAME LAUNCH WRITES WITH PV_SRC_YUV444 AND orient = 0 FOR THE REPLICATED COPY ORIENTED
 *               BEFOREHAND.  (PV_SRC_YUV444 itself keeps the 4:2:0 wording: Y, U and V planes oriented separately.)
 * Kernels:      chroma arrangement and sample width are compiled in, the two shifts are a workgroup-uniform kernel argument:
 *               one kernel serves both layouts (pytorchvideo_amd/csrc/pv_yuv4.hip).  A staged strip or tile holds the luma
 *               span and the chroma span behind it; with full-size chroma that is up to three times the luma bytes.
 * PV_ERR_INVALID, before every HIP call: a pitch that cannot hold a row; a plane outside [0, frame_stride); an odd Ws with
 * PV_SRC_YUV422; c_step outside {1, 2}, or 2 with |v_offset - u_offset| != sb; C != 3; a null yuv2rgb; PV_U16 with an odd
 * address, pitch, offset or stride; an odd rectangle member the subsampling halves; and whatever the entry point rejects of any
 * launch.  PV_ERR_UNSUPPORTED: a staged strip or tile beyond the LDS limit, the index limit of pv_area_views, oriented records
 * in pv_region_views / pv_area_views, pv_hdr_views.  An invalid field wins over an unsupported size.
 */

/* ---- packed YUV 4:2:2: YUY2 / YVYU / UYVY / VYUY and Y210 / Y212 / Y216 frames read where they lie ----------------------------
 * Live sources hand out 4:2:2 in ONE plane: UVC webcams and V4L2 (YUYV), SDI / HDMI capture cards (UYVY), DXVA / VAAPI / Media
 * Foundation for 10- to 16-bit 4:2:2 (Y210 / Y212 / Y216).  Luma and chroma are interleaved in macropixels of four samples, so
 * such a frame needed a de-interleave pass into planes before the launch.  One more value of pv_batch_views_desc.src_layout
 * (declared beside PV_SRC_YUV422; the value 12 is no layout and stays PV_ERR_INVALID) names it:
 *                   PV_SRC_YUYV422   one plane of Hs rows of Ws / 2 macropixels; (csy, csx) = (0, 1), as PV_SRC_YUV422
 * Honoured by:  pv_batch_views, pv_frame_views, pv_region_views and pv_area_views -- whole videos and frame lists, orient 0..7
 *               where the entry point takes it, up to three views, all five destination forms.  pv_box_views reads such
 *               records unchanged.  NOT by pv_hdr_views, which answers PV_ERR_UNSUPPORTED, and not by the one-source entry
 *               points, which have no field for it.
 * Descriptor:   c_step = 4: the samples between x-adjacent samples of one chroma component, which is what c_step counts in
 *               every YUV layout (1 and 2 are PV_ERR_INVALID here, 4 is PV_ERR_INVALID everywhere else).  C = 3; yuv2rgb is
 *               required.  src_dtype PV_U8 (sb = 1) or PV_U16 (sb = 2: little-endian codes; Y210 / Y212 / Y216 keep the value
 *               in the high bits, which lives in yuv2rgb as for every 16-bit layout).
 * Record:       y_pitch: bytes per row, >= 2 * Ws * sb.  c_pitch: 0, as for packed pixels.  frame_stride >= (Hs - 1) * y_pitch +
 *               2 * Ws * sb.  u_offset / v_offset: the byte of the first U / V sample FROM THE START OF A ROW, read per record, so
 *               records of different sample orders share a launch as NV12 and NV21 records do.  Exactly these pairs are valid:
 *                   (sb, 3 sb) YUY2 (Y0 U Y1 V)     (3 sb, sb) YVYU (Y0 V Y1 U)     (0, 2 sb) UYVY (U Y0 V Y1)     (2 sb, 0) VYUY
 *               and luma lies at the other two sample positions:
 *                   U(y, i) = frame[y * y_pitch + u_offset + i * 4 sb]        V likewise        0 <= y < Hs, 0 <= i < Ws / 2
 *                   Y(y, x) = frame[y * y_pitch + y0 + x * 2 sb]              y0 = 0 where U and V are odd samples, else sb
 *                   tap (y, x) uses U(y, x >> 1) and V(y, x >> 1)
 *               Ws is even; any Hs.  PV_U8 frames may start at any byte; PV_U16: the evenness rules of pv_yuv16_views.
 * pv_region_views: left and w are even, as for PV_SRC_YUV422.
 * Arithmetic:   nothing new.  AN ITEM HOLDS, BIT FOR BIT, WHAT THE SAME ENTRY POINT WRITES WITH PV_SRC_YUV422, c_step 1, THE SAME
 *               MATRIX AND THE SAME src_dtype FOR THE PLANAR COPY OF THE SAME FRAMES (Y, U and V planes de-interleaved, nothing
 *               else touched): taps, the per-tap conversion and clamp, the pinned blend, the box filter's windows and summation
 *               order, the affine map and the single rounding are those of that launch, orientation included.
 * Kernels:      pytorchvideo_amd/csrc/pv_yuyv.hip.  A source row is staged ONCE -- the macropixels that cover the span -- and
 *               serves as luma and chroma image both; the sample order is read from the record.
 * PV_ERR_INVALID, before every HIP call: any other (u_offset, v_offset) pair; c_step other than 4; a non-zero c_pitch; an odd Ws;
 * a y_pitch or frame_stride too small; PV_U16 with an odd address, pitch, offset or stride; a rectangle with an odd left or w; C != 3;
 * a null yuv2rgb; and whatever the entry point rejects of any launch.  PV_ERR_UNSUPPORTED: a staged strip or tile beyond the LDS
 * limit, the index limit of pv_area_views, oriented records in pv_region_views / pv_area_views, pv_hdr_views.  An invalid field
 * wins over an unsupported size.
 */

/* ---- key-frame detection: the boxes of a forward mapped into its views, on the device ---------------------------------
 * A detection forward built by pv_batch_views holds one clip per key frame, and every key frame has person boxes given in the
 * pixels of ITS source frame.  pv_box_views fills the RoI head's persistent [capacity][5] fp32 box buffer (what pv_roi_align
 * reads at replay time) for one forward from the box list of the whole call, which was uploaded once: one launch, one thread
 * per destination row, no host arithmetic and no host-to-device copy per forward.
 * Boxes:        boxes[n_boxes][4] fp32 (x1, y1, x2, y2) in source pixels, FINITE (a NaN is not propagated the way
 *               torch.clamp propagates it); box_item[n_boxes] int32, non-decreasing: the position, in the call's item
 *               sequence items_dev[n_seq], of the key frame the box belongs to.
 * Window:       the launch maps boxes [box0, box0 + n_launch) for the forward that holds items [item0, item0 + n_items) of
 *               the sequence -- the window pv_batch_views was given for the same forward, read through the same
 *               sources_dev / items_dev records (Hs, Ws, Hn, Wn, y_off[view], x_off[view]); source and view are clamped
 *               into range before they are used, as pv_batch_views clamps them.
 * Rows:         i < n_launch: {box_item - item0, x1', y1', x2', y2'}; a box whose box_item - item0 is outside [0, n_items)
 *               gets {-1, 0, 0, 0, 0} and nothing is read through it.  n_launch <= i < capacity: {-1, 0, 0, 0, 0}
 *               (pv_roi_align answers zeros for a clip index outside the batch).  dst_box[capacity], when given: box0 + i,
 *               and -1 on the tail.  Nothing beyond `capacity` rows is touched.
 * Arithmetic:   per coordinate, every operation rounded on its own in fp32 (no contraction), shown for x (y: Hs, Hn, y_off,
 *               Ho):  clip_to_source ? v = min(max(v, 0), Ws - 1) : v;
 *                     v = v * r,  r = Ws < Hs ? (float)((double)Hn / (double)Hs) : (float)((double)Wn / (double)Ws);
 *                     v = v - (float)x_off;   v = min(max(v, 0), Wo - 1)
 *               -- clip_boxes_to_image, short_side_scale_with_boxes (ONE ratio, the longer side's, for x and y),
 *               crop_boxes and clip_boxes_to_image of the reference (transforms/functional.py:195-231,407-446), bit for
 *               bit what transforms.boxes_to_view gives on the host.
 * Orientation:  boxes stay pixels of the STORED frame (what a detector that ran on decoder surfaces produces).  For a record
 *               with orient != 0 the box is, after the optional clip_to_source, mapped into the displayed frame D in fp32,
 *               every operation rounded on its own: a mirrored coordinate along an axis of stored length n is
 *               t = (float)n - v; t = t - 1.0f (the reference's `width - boxes - 1` of horizontal_flip_with_boxes,
 *               transforms/functional.py:380-404); rot 1: (x, y) -> (mirror_Hs(y), x); rot 2: (mirror_Ws(x), mirror_Hs(y));
 *               rot 3: (y, mirror_Ws(x)); then the mirror bit: x -> mirror_Wd(x); the corners are re-ordered so that
 *               x1' <= x2' and y1' <= y2'.  The three steps behind run with the displayed Hd / Wd.  Bit for bit
 *               transforms.boxes_to_view(..., orientation=).  An orient outside 0..7 is read as orient & 7.
 * PV_ERR_INVALID: null boxes / box_item / sources_dev / items_dev / dst; capacity, n_items, Ho, Wo, n_sources <= 0;
 * n_views outside 1..3; n_launch < 0 or > capacity; box0 < 0 or box0 + n_launch > n_boxes; item0 < 0 or
 * item0 + n_items > n_seq.  n_launch == 0 is valid and writes only the tail.  Validation precedes every HIP call.
 */
typedef struct pv_box_views_desc {
  const float* boxes;                 /* [n_boxes][4] on the device                                            */
  const int32_t* box_item;            /* [n_boxes] on the device                                               */
  const pv_view_source* sources_dev;  /* [n_sources] on the device: the records pv_batch_views reads           */
  const pv_view_item* items_dev;      /* [n_seq] on the device: the call's WHOLE item sequence                 */
  float* dst;                         /* [capacity][5] on the device                                           */
  int32_t* dst_box;                   /* [capacity] on the device, or NULL                                     */
  int32_t n_boxes, n_seq, n_sources, n_views;
  int32_t box0, n_launch, item0, n_items;
  int32_t Ho, Wo, capacity, clip_to_source;
} pv_box_views_desc;
int pv_box_views(const pv_box_views_desc* d, pv_stream_t stream);

/* ---- row ops on (rows, C) matrices -------------------------------------------------
 * pv_layernorm: nn.LayerNorm(eps) over C (models/vision_transformers.py:333-335,
 *   layers/attention.py:199-205).
 * pv_softmax_rows: nn.Softmax(dim=channel) head activation (models/head.py:384).
 * pv_mean_rows: AdaptiveAvgPool3d(1)+view (models/head.py:386-390): y[b][c] = mean over
 *   `rows_per_batch` rows, fp32 out.
 * pv_add_posenc: SpatioTemporalClsPositionalEncoding.forward
 *   (layers/positional_encoding.py:112-136): writes the cls row and adds the separable
 *   spatial + temporal (+ class) embedding in place.
 */
typedef struct pv_rows_desc {
  const void* x; void* y;
  const float* gamma; const float* beta;  /* layernorm only */
  int64_t rows; int32_t C, ldx, ldy;
  int32_t rows_per_batch;                 /* mean_rows only */
  float eps;
  int32_t dtype;                          /* of x; y same except mean_rows (fp32) */
  int32_t x_f32;                          /* layernorm: 1 = x is fp32 while y is `dtype` */
  int32_t g_period;                       /* layernorm: 0, or gamma/beta are [g_period][C] tables and row r */
                                          /* uses table row r % g_period (per-head norms of several tensors  */
                                          /* packed side by side, layers/attention.py:202-205); C <= 256    */
  int32_t act;                            /* affine_rows only: PV_ACT_* applied after the affine map                */
  int32_t n_prefix;                       /* affine_rows only: the first n_prefix rows of every rows_per_batch block */
                                          /* (the cls token) pass through untouched                                 */
} pv_rows_desc;
int pv_layernorm(const pv_rows_desc* d, pv_stream_t stream);
/* BatchNorm in eval mode on token rows -- the norm="batchnorm" MViT (models/vision_transformers.py:336-339):
 * y[r][c] = act(x[r][c] * gamma[c] + beta[c]) with gamma / beta the folded running statistics.
 *   nn.BatchNorm1d block norms (layers/attention.py:738-753): x fp32 stream (x_f32) -> bf16 GEMM operand;
 *   nn.BatchNorm3d(head_dim) + GELU BEFORE the pooling conv (layers/attention.py:186-190): in place on the q / k / v
 *   columns of the qkv GEMM output (ldx = ldy = row stride, C = heads * head_dim with g_period = 0 and per-channel
 *   tables repeated per head by the caller), cls rows skipped (rows_per_batch, n_prefix).
 * gamma == NULL: scale 1; beta == NULL: shift 0 (a plain fp32 -> bf16 copy of rows, used for the cls rows of a head
 * without a final norm). */
int pv_affine_rows(const pv_rows_desc* d, pv_stream_t stream);
int pv_softmax_rows(const pv_rows_desc* d, pv_stream_t stream);
int pv_mean_rows(const pv_rows_desc* d, pv_stream_t stream);

typedef struct pv_posenc_desc {
  void* x;                    /* [B][1+T*HW][ld] tokens, row 0 = cls (written here) */
  const float* cls_token;     /* [C] or NULL (no cls: rows start at the grid)       */
  const float* pos_spatial;   /* [HW][C]  (separable) or full [T*HW(+1)][C]          */
  const float* pos_temporal;  /* [T][C]  or NULL when pos_spatial is the full table  */
  const float* pos_class;     /* [C] or NULL                                        */
  int32_t B, T, HW, C, ld;
  int32_t dtype;
  int32_t cls_only;           /* 1: write the cls row only (the tables were added by the producing conv) */
} pv_posenc_desc;
int pv_add_posenc(const pv_posenc_desc* d, pv_stream_t stream);

/* ---- fused pooled attention --------------------------------------------------------
 * softmax((q*scale) k^T) v [+ q] of layers/attention.py:531-539 without materialising
 * the scores.  q/k/v/o are token tensors whose channel dim is heads*head_dim
 * (head h at channel offset h*head_dim); fp32 online softmax, MFMA QK^T and PV.
 */
typedef struct pv_attention_desc {
  const void* q; const void* k; const void* v; void* o;
  int64_t q_bs, k_bs, v_bs, o_bs;
  int32_t ldq, ldk, ldv, ldo;
  int32_t B, heads, head_dim, Nq, Nk;
  float scale;          /* finite and > 0, else PV_ERR_INVALID (row maxima are taken before scaling) */
  int32_t residual_q;   /* 1: o += q (residual_pool, layers/attention.py:536-537) */
  int32_t dtype;
} pv_attention_desc;
int pv_attention(const pv_attention_desc* d, pv_stream_t stream);

/* ---- video-level ensembling (the step right after the path) ---------------
 * pytorchvideo_trainer/module/video_classification.py:244-311: preds = softmax(logits) of every clip
 * (30 views per video in the model zoo's test protocol) are summed -- or max-ed -- into its video's
 * score row and the clip is counted: accum[video_index[i]][:] (op)= softmax(logits[i][:]),
 * counts[video_index[i]] += 1, clips taken in index order (deterministic; no atomics).
 * The final division by the count is left to the caller (after the cross-rank reduction).
 */
typedef struct pv_ensemble_desc {
  const float* logits;          /* [N][ld] fp32                                  */
  const int32_t* video_index;   /* [N], each in [0, V)                           */
  float* accum;                 /* [V][C] fp32, updated in place                 */
  int32_t* counts;              /* [V], updated in place                         */
  int32_t N, C, ld, V;
  int32_t mode;                 /* 0 = sum, 1 = max                              */
} pv_ensemble_desc;
int pv_ensemble_scores(const pv_ensemble_desc* d, pv_stream_t stream);

/* ---- elementwise -------------------------------------------------------------------
 * y = act(a + b) over (rows, C): residual joins that cannot ride in a conv epilogue.
 */
typedef struct pv_add_desc {
  const void* a; const void* b; void* y;
  int64_t rows; int32_t C, lda, ldb, ldy;
  int32_t act, dtype;
} pv_add_desc;
int pv_add_act(const pv_add_desc* d, pv_stream_t stream);

/* ---- RoIAlign (+ the whole-window max pool that follows it in the detection head) ---------
 * ResNetRoIHead.forward, models/head.py:437-482: x.squeeze(T) -> roi_layer(x, bboxes) -> pool_spatial.
 * roi_layer is torchvision.ops.RoIAlign (a third-party op, default of create_res_roi_pooling_head,
 * models/head.py:212): for box n = (batch index, x1, y1, x2, y2) and output bin (ph, pw) the mean of
 * grid_h x grid_w bilinear samples of the feature map, grid = sampling_ratio, or ceil(roi size / bins)
 * when sampling_ratio <= 0; `aligned` = 0 is torchvision's default (no half-pixel shift, roi size >= 1).
 * pool_max = 1 additionally takes the maximum over all ph x pw bins (MaxPool2d(resolution, stride=1),
 * models/head.py:317) and writes one row per box: the [R, C, ph, pw] tensor is never stored.
 * Boxes are read on the device at launch time (their VALUES may change between graph replays, their
 * count may not).  A box whose batch index is outside [0, B) produces zeros.
 */
typedef struct pv_roi_align_desc {
  const void* x;        /* [B][H][W][ldx] features (temporal dim already pooled to 1) */
  const float* boxes;   /* [R][5] fp32: batch index, x1, y1, x2, y2 in input-image pixels */
  void* y;              /* pool_max ? [R][ldy] : [R][ph][pw][ldy]                     */
  int64_t x_bs;         /* elements between batch items of x                          */
  int32_t ldx, ldy;
  int32_t B, H, W, C, R;
  int32_t ph, pw;       /* output resolution (head_spatial_resolution)               */
  int32_t sampling_ratio, aligned, pool_max;
  float spatial_scale;
  int32_t dtype;        /* storage type of x and y                                    */
} pv_roi_align_desc;
int pv_roi_align(const pv_roi_align_desc* d, pv_stream_t stream);

/* ---- X3D bottleneck block, fully fused (round 6) ------------------------------------------------------------
 * Replaces a whole residual block without squeeze-excitation -- pytorchvideo/models/x3d.py:169-212
 * (create_x3d_bottleneck_block: conv_a 1x1x1 + norm_a + ReLU, conv_b depthwise 3x3x3 + norm_b + Swish, conv_c 1x1x1 + norm_c),
 * models/resnet.py:1345-1365 (BottleneckBlock.forward) and :1179-1189 (ResBlock.forward: + shortcut, activation) -- in ONE launch
 * that never writes the expanded tensor (csrc/pv_block.hip):
 *     y = act_out( r + sc * (Wc . act_b( sb * dw3x3x3( act_a( sa * (Wa . x) + ha ) ) + hb )) + hc )
 * x (B, T, H, W, cin), r = residual (B, T, H, W, cout) or NULL, y (B, T, H, W, cout): bf16 channels-last, all strides 1,
 * the depthwise conv zero-pads the EXPANDED tensor by 1 on every side.  Host-packed operands (Cp = round_up(C, 32),
 * cin_p = round_up(cin, 32)):
 *   wa  [Cp/16][cin_p/32][64 lanes][8] bf16   Wa[16 mt + (l&15)][32 ks + 8 (l>>4) + j]   (zeros beyond C / cin)
 *   wb  [27][Cp] fp32                         depthwise taps, t = (kt*3 + kh)*3 + kw
 *   wc  [cout/16][Cp/32][64 lanes][8] bf16    Wc[16 mt + (l&15)][32 ks + 8 (l>>4) + j]   (zeros beyond C)
 *   sa, ha, sb, hb [Cp] fp32; sc, hc [cout] fp32: the folded BatchNorms (zeros in the padding channels)
 * (pytorchvideo_amd/accelerator/mi355x/emit.py::emit_fused_bottleneck packs them.)  pv_bottleneck_supported(d) == 1 for the
 * geometries the kernel is instantiated for: W <= 14, X3D res4 (cin 96, C 216, cout 96). */
typedef struct pv_bottleneck_desc {
  const void* x; void* y; const void* residual;
  const void* wa; const float* wb; const void* wc;
  const float* sa; const float* ha; const float* sb; const float* hb; const float* sc; const float* hc;
  int64_t x_bs, y_bs, r_bs;          /* batch strides, elements */
  int32_t ldx, ldy, ldr;             /* voxel strides, elements */
  int32_t B, T, H, W;
  int32_t cin, C, cout;              /* true channel counts */
  int32_t act_a, act_b, act_out;     /* pv_act after norm_a / norm_b / the residual join */
  int32_t dtype;                     /* PV_BF16 */
  /* mode PV_BLOCK_AB -- blocks WITH squeeze-excitation (x3d.py:190-207: norm_b = Sequential(BN, SE)): the launch stops behind
   * conv_b.  y receives  sb * dw3x3x3(act_a(...)) + hb  (no activation: conv_c applies gate and Swish while loading its operand)
   * as bf16 (B, T, H, W, C) with voxel stride ldy, and psum[b][blk][round_up(C, 8)] (fp32, blk < pv_bottleneck_psum_blocks(d))
   * the sums of those values over the block's voxels -- the squeeze of fvcore's SqueezeExcitation, one writer per entry, no
   * atomics; pv_se_gate turns them into the gate.  wc, sc, hc, residual, cout, act_b, act_out are ignored. */
  int32_t mode;
  float* psum;
} pv_bottleneck_desc;
#define PV_BLOCK_FULL 0
#define PV_BLOCK_AB 1
int pv_bottleneck(const pv_bottleneck_desc* d, pv_stream_t stream);
int pv_bottleneck_supported(const pv_bottleneck_desc* d);
int pv_bottleneck_psum_blocks(const pv_bottleneck_desc* d);

/* ---- fused MLP of a MultiScaleBlock on token rows -------------------------------------------------------
 * Replaces  norm2 -> Mlp.fc1 -> GELU -> Mlp.fc2 -> + residual  (pytorchvideo/layers/attention.py:102-114 Mlp.forward,
 * :750-757 the block's second half) in ONE launch whose hidden tensor never leaves the chip (csrc/pv_mlp.hip):
 *     y[m][:] = R[m][:] + b2 + W2 . act(W1 . xn[m][:] + b1)
 *   ln_gamma != NULL:  x is the fp32 token stream [M][ldx]; xn = LayerNorm(x; ln_gamma, ln_beta, ln_eps) is computed
 *                      in the kernel and R = x (the row is read once); needs C == Cout, residual == NULL.
 *   ln_gamma == NULL:  x is a bf16 operand tensor [M][ldx] (the LayerNorm output); R = residual (fp32 [M][ldr]) or 0.
 * y is fp32 [M][ldy].  dtype must be PV_BF16 (weights bf16, fp32 accumulation / bias / activation / LayerNorm).
 * `w12` is the host-packed LDS image the kernel streams: H/32 + 1 blocks of  C/16*1024 + Cout/32*2048 + 256  bytes, block j
 * holding W1 of hidden block j and W2 of hidden block j - 1 (the kernel multiplies phase B one block behind phase A so that the
 * activation issues in the shadow of MFMAs; W2 of block -1, W1 and b1 of block H/32 are zeros), FOLLOWED BY TWO MORE BLOCKS OF
 * PADDING (any finite values; the kernel prefetches two blocks ahead without a branch).  Block j, in fragments of
 * v_mfma_f32_16x16x32_bf16 (round 6: 16 token rows per wave, lane l = 16 g + m):
 *   [f = 2 ks + uh < C/16][l < 64][j8 < 8]  bf16  W1[32 j + 16 uh + (l&15)][32 ks + 8 (l>>4) + j8]
 *   [ob < Cout/16][l < 64][j8 < 8]          bf16  W2[32 (ob>>1) + 8 ((l&15)>>2) + 4 (ob&1) + (l&3)][32 (j-1) + u(l>>4, j8)],
 *        u(g, j8) = j8 < 4 ? 4 g + j8 : 16 + 4 g + j8 - 4
 *   [u < 32] fp32  b1[32 j + u]  (zeros when the layer has no bias), then 128 bytes of padding
 * (pytorchvideo_amd/accelerator/mi355x/emit_mvit.py::pack_mlp_weights builds it).  b2 is [Cout] fp32 or NULL.
 * pv_mlp_rows_supported(d) == 1 for the (C, Cout) pairs the kernel is instantiated for (MViT-B: 96/192, 192/192,
 * 192/384, 384/384; H any multiple of 32). */
typedef struct pv_mlp_desc {
  const void* x;
  const void* w12;
  void* y;
  const float* b2;
  const float* residual;
  const float* ln_gamma;
  const float* ln_beta;
  int64_t M;             /* token rows */
  int32_t C, H, Cout;    /* in / hidden / out widths */
  int32_t ldx, ldr, ldy; /* row strides, elements */
  int32_t act;           /* pv_act between the two Linears */
  int32_t dtype;         /* PV_BF16 */
  float ln_eps;
  /* Optional (round 4): yn != NULL -> the kernel ALSO writes yn[m][:] = LayerNorm(y[m][:]; nn_gamma, nn_beta, nn_eps) as
   * bf16 [M][ldyn] from the rows it still holds in registers: norm1 of the NEXT MultiScaleBlock (layers/attention.py:729-737),
   * i.e. the operand of that block's q|k|v projection, without a LayerNorm launch reading the stream back. */
  void* yn;
  const float* nn_gamma;
  const float* nn_beta;
  int32_t ldyn;
  float nn_eps;
} pv_mlp_desc;
int pv_mlp_rows(const pv_mlp_desc* d, pv_stream_t stream);
int pv_mlp_rows_supported(const pv_mlp_desc* d);

/* ---- LayerNorm + Linear on token rows ----------------------------------------------------------------------
 * Replaces  norm1 -> the q | k | v Linear(s)  of MultiScaleBlock / MultiScaleAttention (pytorchvideo/layers/attention.py:
 * 729-737 norm1, :425-451 _qkv_proj; the three Linears concatenated along the output dim) in ONE launch:
 *     y[m][:] = act( W . LayerNorm(x[m][:]; ln_gamma, ln_beta, ln_eps) + b )
 * x is the fp32 token stream [M][ldx], y is bf16 [M][ldy]; the bf16 operand tensor between LayerNorm and the GEMM is
 * never written.  `wb` is the host-packed per-output-block LDS image, N/32 blocks of  C/16*1024 + 256  bytes followed
 * by two more blocks of padding (prefetched, never used):
 *   [ks < C/16][hi < 2][rho < 32][j < 8]  bf16  W[32 nb + chi(rho)][32 (ks>>1) + 16 hi + 8 (ks&1) + j]   (chi as above)
 *   [hi < 2][r < 16]  fp32  b[32 nb + 16 hi + r]  (zeros without bias), then 128 bytes of padding
 * (pytorchvideo_amd/accelerator/mi355x/emit_mvit.py::pack_ln_linear_weights).  C in {96, 192, 384, 768}, N % 32 == 0. */
typedef struct pv_ln_linear_desc {
  const void* x;
  const void* wb;
  void* y;
  const float* ln_gamma;
  const float* ln_beta;
  int64_t M;
  int32_t C, N;
  int32_t ldx, ldy;
  int32_t act;
  int32_t dtype;         /* PV_BF16 */
  float ln_eps;
} pv_ln_linear_desc;
int pv_ln_linear_rows(const pv_ln_linear_desc* d, pv_stream_t stream);
int pv_ln_linear_rows_supported(const pv_ln_linear_desc* d);

/* ---- execution plan ----------------------------------------------------------------
 * A deploy-form model is specialised to one input size (reference contract:
 * accelerator/deployment/mobile_cpu/utils/model_conversion.py:100-103), so its forward
 * is a fixed launch list.  The plan records descriptors once; pv_plan_launch replays them
 * from C++ (no Python per layer), optionally through a captured hipGraph.
 */
enum pv_op_kind {
  PV_OP_CONV3D = 1, PV_OP_DWCONV3D = 2, PV_OP_SE_GATE = 3, PV_OP_POOL3D = 4,
  PV_OP_LAYERNORM = 5, PV_OP_SOFTMAX_ROWS = 6, PV_OP_MEAN_ROWS = 7, PV_OP_POSENC = 8,
  PV_OP_ATTENTION = 9, PV_OP_ADD_ACT = 10, PV_OP_INGEST = 11, PV_OP_EGRESS = 12, PV_OP_TOKEN_POOL = 13,
  PV_OP_ROI_ALIGN = 14, PV_OP_LATERAL = 15, PV_OP_AFFINE_ROWS = 16, PV_OP_MLP_ROWS = 17, PV_OP_LN_LINEAR = 18,
  PV_OP_BOTTLENECK = 19
};
typedef struct pv_plan pv_plan;
pv_plan* pv_plan_create(void);
void pv_plan_destroy(pv_plan* p);
int pv_plan_add(pv_plan* p, int op_kind, const void* desc, size_t desc_bytes); /* returns op index */
int pv_plan_size(const pv_plan* p);
int pv_plan_launch(pv_plan* p, pv_stream_t stream);                 /* eager replay   */
int pv_plan_launch_range(pv_plan* p, int first, int last, pv_stream_t stream);
int pv_plan_graph_build(pv_plan* p, pv_stream_t stream);           /* capture+instantiate */
int pv_plan_graph_launch(pv_plan* p, pv_stream_t stream);
/* `n` independent plans (sub-batches of one forward: pytorchvideo_amd.accelerator.mi355x.conversion.SplitBatchDeployed)
 * captured as `n` PARALLEL branches of ONE graph: the runtime runs the branches side by side, so the tail of one
 * sub-batch's kernel overlaps the other's work.  The joint graph is its OWN object (round 3): it does not live in,
 * and is not disturbed by, the graph slot of any member plan (pv_plan_graph_build on a member leaves it intact);
 * rebuild it after pv_plan_add on a member.  Replaces the Python loop over sub-batches; the reference has no
 * counterpart (its forward is one ATen call sequence per batch, models/net.py:41-44). */
typedef struct pv_joint pv_joint;
pv_joint* pv_joint_create(void);
void pv_joint_destroy(pv_joint* j);
int pv_joint_build(pv_joint* j, pv_plan* const* plans, int n);     /* capture + instantiate, 1 <= n <= 16 */
int pv_joint_launch(pv_joint* j, pv_stream_t stream);
int pv_joint_branches(const pv_joint* j);                          /* 0 until built */
/* per-op device time in ms: every op timed in situ between its own pair of HIP events on `stream`, behind a
 * queued un-instrumented replay (the host never paces the measurement); minimum over `iters` passes, minus the
 * null interval of an empty event pair */
int pv_plan_profile(pv_plan* p, pv_stream_t stream, int iters, float* ms_per_op);
/* symbol of the kernel op `i` was routed to ("gemm_glds_kernel", "pw_stream_kernel", ...; the last one when an op launches
 * several), known after pv_plan_profile ran; "" before.  The string lives as long as the plan. */
const char* pv_plan_op_kernel(const pv_plan* p, int i);

/* ---- head collective ----------------------------------------------------------------------
 * The one exchange of the batch-sharded forward: every rank contributes its [B_local, classes] logits and obtains
 * the [B_global, classes] rows (the reference's forward has no collective, models/net.py:41-44; BASELINE.json
 * prescribes this one on the classification head, models/head.py:376-382).  The library binds RCCL itself
 * (dlopen of librccl: ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy / ncclGetErrorString)
 * and ENQUEUES the all-gather from C on the stream the forward was launched on, directly behind the graph
 * launch -- no Python, no torch.distributed call per step.  Bootstrap: rank 0 makes the 128-byte id
 * (pv_comm_unique_id), the host side hands it to every rank (any out-of-band channel; pytorchvideo_amd.parallel
 * uses the process group's store), every rank calls pv_comm_create.
 *   lib_paths: ':'-separated candidates for librccl, tried in order (a copy already mapped into the process --
 *   torch's -- is preferred so that one RCCL instance serves both); NULL = "librccl.so:librccl.so.1".
 * pv_comm_all_gather(send, recv, bytes_per_rank): recv[r*bytes .. (r+1)*bytes) = rank r's send; byte-typed (ncclUint8),
 * asynchronous on `stream`, safe behind pv_plan_graph_launch / pv_joint_launch on the same stream.
 * pv_forward_gather: ONE C call per step of the batch-sharded forward (what a step of `bench.py --gpus N` is):
 *   graph launch (plan `p`, or joint graph `j` -- exactly one non-NULL) -> the rank's logits rows collected from up to
 *   16 strided sources (the result buffers of the sub-batch plans) into `staging` -> all-gather into `recv`
 *   ([world][bytes_per_rank], i.e. the [B_global, classes] rows), all enqueued on `stream`.
 *   c == NULL or world 1: the rows are collected straight into `recv` (no RCCL call). */
typedef struct pv_comm pv_comm;
typedef struct pv_gather_src {
  const void* ptr;     /* first row                         */
  size_t row_bytes;    /* bytes copied per row              */
  size_t row_pitch;    /* bytes between rows (>= row_bytes)  */
  int64_t rows;
} pv_gather_src;
int pv_comm_probe(const char* lib_paths);          /* PV_OK when a librccl with the five entry points can be bound */
int pv_comm_unique_id(void* id128, const char* lib_paths);
int pv_comm_create(pv_comm** out, const void* id128, int rank, int world, const char* lib_paths);
void pv_comm_destroy(pv_comm* c);
int pv_comm_rank(const pv_comm* c);
int pv_comm_world(const pv_comm* c);
const char* pv_comm_library(const pv_comm* c);     /* path of the RCCL copy the communicator bound */
int pv_comm_all_gather(pv_comm* c, const void* send, void* recv, size_t bytes_per_rank, pv_stream_t stream);
int pv_forward_gather(pv_plan* p, pv_joint* j, pv_comm* c, const pv_gather_src* srcs, int n_srcs, void* staging,
                      void* recv, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PV_MI355X_H_ */
