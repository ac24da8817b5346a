// pv_yuv_views: pv_video_views on decoder-native YUV 4:2:0 frames (NV12 / NV21: one interleaved chroma plane, c_step 2;
// I420 / YV12: two chroma planes, c_step 1).  The arithmetic is pinned in include/pv_mi355x.h: every TAP is converted to
// RGB in registers (three fused multiply-adds per channel, clamped to [0, 255]), then blended, mapped and stored as
// pv_resample_crop does.  No RGB frame exists anywhere.
//
// The kernel is the staged strip of pv_rs.h (rs_strip_yuv: stage, barrier, gather) on a geometry taken from the by-value
// descriptor; this file holds the descriptor's validation.
//
// pv_yuv16_views is the same on 16-bit little-endian samples (P010 / P012 / P016, yuv420p10le and kin): the same descriptor
// with pitches, offsets and the frame stride still in bytes, the same body instantiated for two-byte samples in kernels of
// their own (yuv16_views_kernel), and the evenness checks that keep its 16-bit LDS reads aligned.  Depth and bit alignment
// live in the caller's matrix.
#include "pv_rs.h"

namespace {

struct YuvLaunch {
  float sy, sx;          // (float)Hs / (float)Hn, (float)Ws / (float)Wn: divided once, on the host
  int32_t R;             // output rows per workgroup
  int32_t pitch_y;       // LDS bytes per staged luma row: multiple of 16, >= 15 + widest span
  int32_t pitch_c;       // LDS bytes per staged chroma (row, plane)
  int32_t c_base;        // LDS offset of the chroma image: 2 R pitch_y
};

// CSTEP / FORM / D: as rs_strip_yuv.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv_views_kernel(const pv_yuv_views_desc d, const YuvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char yv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const int item = d.item0 + zi;
  const int clip = item / d.n_views, view = item - clip * d.n_views;
  RsYuvSrc s;
  s.src = reinterpret_cast<uintptr_t>(d.src);
  // clamped before any address is formed: a malformed table can never read outside the source
  s.frame_off = (long)min(max(d.t_index[(long)clip * d.t_stride + t], 0), d.N - 1) * d.frame_stride;
  s.Hs = d.Hs, s.Ws = d.Ws;
  s.sy = g.sy, s.sx = g.sx;
  s.yoff = rs_view_off(view, d.y_off[0], d.y_off[1], d.y_off[2]);
  s.xoff = rs_view_off(view, d.x_off[0], d.x_off[1], d.x_off[2]);
  s.y_pitch = d.y_pitch, s.c_pitch = d.c_pitch;
  rs_chroma_planes(CSTEP == 2, d.u_offset, d.v_offset, s);
  rs_strip_yuv<CSTEP, FORM, D>(yv_lds, g.R, g.pitch_y, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, false);
}

// The same on two-byte samples (PV_U16 / pv_yuv16_views).  A kernel of its own, spelled out rather than sharing a wrapper
// with the one above: routed through a common inline function the 8-bit kernels come out with other instructions than
// they had (commuted scalar adds), and their code is pinned.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv16_views_kernel(const pv_yuv_views_desc d, const YuvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char yv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const int item = d.item0 + zi;
  const int clip = item / d.n_views, view = item - clip * d.n_views;
  RsYuvSrc s;
  s.src = reinterpret_cast<uintptr_t>(d.src);
  // clamped before any address is formed: a malformed table can never read outside the source
  s.frame_off = (long)min(max(d.t_index[(long)clip * d.t_stride + t], 0), d.N - 1) * d.frame_stride;
  s.Hs = d.Hs, s.Ws = d.Ws;
  s.sy = g.sy, s.sx = g.sx;
  s.yoff = rs_view_off(view, d.y_off[0], d.y_off[1], d.y_off[2]);
  s.xoff = rs_view_off(view, d.x_off[0], d.x_off[1], d.x_off[2]);
  s.y_pitch = d.y_pitch, s.c_pitch = d.c_pitch;
  rs_chroma_planes(CSTEP == 2, d.u_offset, d.v_offset, s);
  rs_strip_yuv<CSTEP, FORM, D, unsigned short>(yv_lds, g.R, g.pitch_y, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, false);
}

// sb: bytes per sample, 1 (pv_yuv_views) or 2 (pv_yuv16_views).
int yuv_run(pv_yuv_views_desc d, pv_stream_t stream, int sb) {
  if (d.n_clips <= 0 || d.T <= 0 || d.N <= 0 || d.Hs <= 0 || d.Ws <= 0 || d.Hn <= 0 || d.Wn <= 0 || d.Ho <= 0 || d.Wo <= 0)
    return PV_ERR_INVALID;
  if (d.t_stride < d.T) return PV_ERR_INVALID;
  if (int e = rs_check_yuv_planes(d.Hs, d.Ws, d.c_step, d.y_pitch, d.c_pitch, d.frame_stride, d.u_offset, d.v_offset, sb)) return e;
  if (sb == 2)
    if (int e = rs_check_yuv16_even(reinterpret_cast<uintptr_t>(d.src), d.y_pitch, d.c_pitch, d.frame_stride, d.u_offset, d.v_offset))
      return e;
  if (int e = rs_check_views(d.n_views, d.y_off, d.x_off, d.Ho, d.Wo, d.Hn, d.Wn)) return e;
  if (int e = rs_check_items(d.item0, d.n_items, (long)d.n_clips * d.n_views, d.T)) return e;
  if (int e = rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo)) return e;

  YuvLaunch g;
  g.sy = (float)d.Hs / (float)d.Hn;
  g.sx = (float)d.Ws / (float)d.Wn;
  // the widest luma and chroma column spans of any view size the staged rows
  int span_y = 0, span_c = 0;
  rs_widest_span(g.sx, d.x_off, d.n_views, d.Wo, d.Ws, span_y, span_c);
  // two source rows per output row, each with its chroma
  size_t lds;
  if (int e = rs_strip_rows(rs_yuv_pitches(span_y, span_c, d.c_step, sb, g.pitch_y, g.pitch_c), d.Ho, g.R, lds)) return e;
  g.c_base = 2 * g.R * g.pitch_y;
#define YV_STRIPS(KERNEL, CSTEP) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), KERNEL, CSTEP)
  if (sb == 2) {
    if (d.c_step == 2) YV_STRIPS(yuv16_views_kernel, 2);
    else YV_STRIPS(yuv16_views_kernel, 1);
  } else {
    if (d.c_step == 2) YV_STRIPS(yuv_views_kernel, 2);
    else YV_STRIPS(yuv_views_kernel, 1);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_yuv_views(const pv_yuv_views_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->src || !dp->dst || !dp->t_index || !dp->yuv2rgb) return PV_ERR_INVALID;
  return yuv_run(*dp, stream, 1);
}

extern "C" int pv_yuv16_views(const pv_yuv_views_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->src || !dp->dst || !dp->t_index || !dp->yuv2rgb) return PV_ERR_INVALID;
  return yuv_run(*dp, stream, 2);
}
