// pv_resample_crop: short_side_scale + uniform_crop (reference transforms/functional.py:92-131,302-347) fused with the
// ingest's frame selection, Div255 + Normalize affine, dtype conversion and layout change.
// pv_video_views: the same kernel reading ONE video through a frame table with a row per clip -- the clip sampler,
// FrameVideo.get_clip (data/frame_video.py:149-200) and UniformTemporalSubsample of the reference's data pipeline as data.
//
// The kernel is the staged strip of pv_rs.h (rs_strip_rgb: stage, barrier, gather) on a geometry taken from the by-value
// descriptor; this file holds the descriptor's validation and the frame selection of the two entry points.
#include "pv_rs.h"

namespace {

struct RsLaunch {
  float sy, sx;     // (float)Hs / (float)Hn, (float)Ws / (float)Wn: divided once, on the host
  int32_t R;        // output rows per workgroup
  int32_t pitch;    // LDS bytes per staged (row, plane): multiple of 16, >= 15 + widest span
  int32_t src_T;    // frames per source plane; every selected frame is clamped into [0, src_T - 1]
  int32_t item0;
  int32_t tab_stride;   // t_index row stride per clip: 0 = one row shared by all clips (pv_resample_crop)
  int64_t clip_frames;  // frames from one source clip to the next: 0 = every clip reads the one video (pv_video_views)
};

// S / INTER / FORM / D: as rs_strip_rgb.
// Source clip b starts g.clip_frames frames behind clip b - 1 and takes its frames from row b * g.tab_stride of d.t_index:
// B clips with one shared row (pv_resample_crop), or one video with a row per clip (pv_video_views: clip_frames == 0).
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void resample_crop_kernel(const pv_resample_desc d, const RsLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const int item = g.item0 + zi;
  const int b = item / d.n_views, view = item - b * d.n_views;
  RsRgbSrc s;
  s.src = reinterpret_cast<uintptr_t>(d.src);
  s.Hs = d.Hs, s.Ws = d.Ws, s.N = g.src_T;
  s.sy = g.sy, s.sx = g.sx;
  s.yoff = rs_view_off(view, d.y_off[0], d.y_off[1], d.y_off[2]);
  s.xoff = rs_view_off(view, d.x_off[0], d.x_off[1], d.x_off[2]);
  // a null table selects frame t; clamped: a malformed table can never read outside the source
  s.ts = min(max(d.t_index ? d.t_index[(long)b * g.tab_stride + t] : t, 0), g.src_T - 1);
  s.clip_frame0 = (long)b * g.clip_frames;
  rs_strip_rgb<S, INTER, FORM, D>(rs_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, false);
}

// Validation and launch shared by both entry points.  `one_video`: the source is one video [C,src_T,Hs,Ws] / [src_T,Hs,Ws,3]
// every clip reads through its own row of t_index (row stride tab_stride); else B clips and one shared t_index row.
int rs_run(pv_resample_desc d, bool one_video, int tab_stride, pv_stream_t stream) {
  if (d.B <= 0 || d.C <= 0 || d.T <= 0 || d.Hs <= 0 || d.Ws <= 0 || d.Hn <= 0 || d.Wn <= 0 || d.Ho <= 0 || d.Wo <= 0)
    return PV_ERR_INVALID;
  if (d.C > 4) return PV_ERR_INVALID;
  if (int e = rs_check_views(d.n_views, d.y_off, d.x_off, d.Ho, d.Wo, d.Hn, d.Wn)) return e;
  if (d.src_layout != PV_SRC_NCTHW && d.src_layout != PV_SRC_NTHWC) return PV_ERR_INVALID;
  if (d.src_layout == PV_SRC_NTHWC && (d.src_dtype != PV_U8 || d.C != 3)) return PV_ERR_INVALID;
  if (d.t_index && d.src_T <= 0) return PV_ERR_INVALID;
  if (one_video && (!d.t_index || tab_stride < d.T)) return PV_ERR_INVALID;
  if (int e = rs_check_items(d.item0, d.n_items, (long)d.B * d.n_views, d.T)) return e;
  // the dtype / layout matrix
  if (d.src_dtype != PV_U8 && d.src_dtype != PV_F32) return PV_ERR_UNSUPPORTED;
  if (int e = rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo)) return e;
  if (d.src_dtype == PV_F32 && reinterpret_cast<uintptr_t>(d.src) % 4) return PV_ERR_INVALID;

  RsLaunch g;
  g.sy = (float)d.Hs / (float)d.Hn;
  g.sx = (float)d.Ws / (float)d.Wn;
  g.src_T = d.t_index ? d.src_T : d.T;
  g.item0 = d.item0;
  g.tab_stride = one_video ? tab_stride : 0;
  g.clip_frames = one_video ? 0 : (int64_t)(d.src_layout == PV_SRC_NTHWC ? 1 : d.C) * g.src_T;
  // the widest column span of any view sizes the staged row
  const bool inter = d.src_layout == PV_SRC_NTHWC;
  int span = 0, span_c = 0;
  rs_widest_span(g.sx, d.x_off, d.n_views, d.Wo, d.Ws, span, span_c);
  g.pitch = rs_rgb_pitch(span, d.src_layout, d.src_dtype);
  size_t lds;
  if (int e = rs_strip_rows(2L * (inter ? 1 : d.C) * g.pitch, d.Ho, g.R, lds)) return e;   // two source rows per output row
#define RC_STRIPS(S, INTER) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), resample_crop_kernel, S, INTER)
  if (inter) RC_STRIPS(unsigned char, true);
  else if (d.src_dtype == PV_U8) RC_STRIPS(unsigned char, false);
  else RC_STRIPS(float, false);
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_resample_crop(const pv_resample_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->src || !dp->dst) return PV_ERR_INVALID;
  return rs_run(*dp, false, 0, stream);
}

// One video, one frame table: the same kernel with B = n_clips, src_T = N and a table row per clip.
extern "C" int pv_video_views(const pv_video_views_desc* vp, pv_stream_t stream) {
  if (!vp || !vp->src || !vp->dst) return PV_ERR_INVALID;   // n_clips, T, N, the table and its stride: rs_run (B, T, src_T)
  pv_resample_desc d = {};
  d.src = vp->src; d.dst = vp->dst;
  d.B = vp->n_clips; d.C = vp->C; d.T = vp->T;
  d.src_T = vp->N; d.Hs = vp->Hs; d.Ws = vp->Ws;
  d.src_dtype = vp->src_dtype; d.src_layout = vp->src_layout;
  d.Hn = vp->Hn; d.Wn = vp->Wn; d.Ho = vp->Ho; d.Wo = vp->Wo;
  d.n_views = vp->n_views;
  for (int v = 0; v < 3; ++v) { d.y_off[v] = vp->y_off[v]; d.x_off[v] = vp->x_off[v]; }
  d.item0 = vp->item0; d.n_items = vp->n_items;
  d.dst_layout = vp->dst_layout; d.dst_dtype = vp->dst_dtype;
  d.c_p = vp->c_p; d.ld = vp->ld; d.bs = vp->bs;
  d.t_index = vp->t_index; d.ch_scale = vp->ch_scale; d.ch_shift = vp->ch_shift;
  return rs_run(d, true, vp->t_stride, stream);
}
