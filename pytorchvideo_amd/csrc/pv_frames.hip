// pv_frame_views: pv_batch_views with every FRAME individually addressed.  A hardware decoder hands out surfaces from a pool
// -- one allocation per frame, uniform geometry and pitch, any order, reused -- and a live stream never is one tensor; here
// a source is a slice of a device table of frame base addresses instead of one allocation with a constant frame stride.
//
// The kernels are the staged strips of pv_rs.h (rs_strip_rgb, rs_strip_yuv), wrapped as pv_batch.hip wraps them: blockIdx.z
// loads its 16-byte item, clamps source / row / view into range, loads the item's record and clamps the table entry into
// [0, N-1] of that source.  Where batch_views_kernel multiplies the entry by the frame size, these load the frame's base
// address from the record's slice (record.src + 8 * entry) -- one more workgroup-uniform, scalar load -- and hand the
// body a geometry with the frame at offset 0: a one-frame source (N = 1, ts = 0) for the RGB / planar forms, frame_off = 0
// for YUV.  Every other value the body sees is the one batch_views_kernel gives it, so an item holds the bits
// pv_batch_views writes for the same frames in one allocation.  The body fetches only the aligned 16-byte granules that
// cover a byte of the span, and such a granule lies in the page of that byte: a frame that ends at the end of its
// allocation is safe.
//
// What stays per launch -- R, the LDS pitch(es) -- is sized as pv_batch_views sizes it, from the host copies of the records
// the items name.  The descriptor embeds a whole pv_batch_views_desc; its checks are repeated here (pv_batch.hip keeps its
// own in its anonymous namespace) with the record's `src` read as a table slice.
//
// PV_U16 sources (16-bit YUV samples) are validated and sized here and launched from pv_frames16.hip, which holds their
// kernels: this translation unit keeps exactly its 25.
#include <cstring>

#include "pv_frames.h"

namespace {

// S / INTER / FORM / D: as rs_strip_rgb.  One frame is a dense [C, Hs, Ws] (plane stride of ONE frame) or [Hs, Ws, 3].
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void frame_views_kernel(const pv_batch_views_desc d, const FvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const FvItem item = fv_item(d, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsRgbSrc s;
  s.src = item.frame;
  s.Hs = V->Hs, s.Ws = V->Ws, s.N = 1;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.ts = 0;
  s.clip_frame0 = 0;
  rs_strip_rgb<S, INTER, FORM, D>(fv_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, true);
}

// CSTEP / FORM / D: as rs_strip_yuv.  One frame is one surface: the record's offsets and pitches, from the frame's base.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void frame_yuv_kernel(const pv_batch_views_desc d, const FvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fy_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const FvItem item = fv_item(d, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = item.frame;
  s.frame_off = 0;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  rs_strip_yuv<CSTEP, FORM, D>(fy_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// One record of a launch: a slice [k, k + N) of the pointer table whose entries are frames (non-null; fp32: 4-byte
// aligned), positive sizes, windows inside the scaled frame, sy / sx the library's own division, and for YUV the planes
// inside one frame.
int fv_check_record(const pv_frame_views_desc& f, const pv_view_source& v, bool yuv) {
  const pv_batch_views_desc& d = f.batch;
  if (!v.src || v.N <= 0 || v.Hs <= 0 || v.Ws <= 0 || v.Hn <= 0 || v.Wn <= 0) return PV_ERR_INVALID;
  const uintptr_t base = reinterpret_cast<uintptr_t>(f.frame_ptrs_dev), at = reinterpret_cast<uintptr_t>(v.src);
  if (at < base || (at - base) % 8) return PV_ERR_INVALID;
  const uint64_t k = (at - base) / 8;
  if (k + (uint64_t)v.N > (uint64_t)f.n_frame_ptrs) return PV_ERR_INVALID;
  const bool f32 = !yuv && d.src_dtype == PV_F32, u16 = yuv && d.src_dtype == PV_U16;
  for (int i = 0; i < v.N; ++i) {
    const uint64_t p = f.frame_ptrs[k + i];
    if (!p || (f32 && p % 4) || (u16 && !rs_yuv16_even((uintptr_t)p))) return PV_ERR_INVALID;
  }
  if (int e = rs_check_views(d.n_views, v.y_off, v.x_off, d.Ho, d.Wo, v.Hn, v.Wn)) return e;
  if (!same_bits(v.sy, (float)v.Hs / (float)v.Hn) || !same_bits(v.sx, (float)v.Ws / (float)v.Wn)) return PV_ERR_INVALID;
  if (yuv) {
    if (int e = rs_check_yuv_planes(v.Hs, v.Ws, d.c_step, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset, u16 ? 2 : 1))
      return e;
    if (u16) return rs_check_yuv16_even(0, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset);   // frames: above
  }
  return PV_OK;
}

int fv_run(const pv_frame_views_desc& f, pv_stream_t stream) {
  const pv_batch_views_desc& d = f.batch;
  if (!d.sources || !d.sources_dev || !d.items || !d.items_dev || !d.t_index || !d.dst) return PV_ERR_INVALID;
  if (!f.frame_ptrs || !f.frame_ptrs_dev || f.n_frame_ptrs <= 0) return PV_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(f.frame_ptrs_dev) % 8) return PV_ERR_INVALID;
  if (d.n_sources <= 0 || d.n_items <= 0 || d.n_rows <= 0 || d.T <= 0 || d.C <= 0 || d.Ho <= 0 || d.Wo <= 0) return PV_ERR_INVALID;
  if (d.t_stride < d.T || d.n_items > 65535 || d.T > 65535) return PV_ERR_INVALID;   // grid.y / grid.z
  if (d.C > 4 || d.n_views < 1 || d.n_views > 3) return PV_ERR_INVALID;
  const bool yuv = d.src_layout == PV_SRC_YUV420;
  if (!yuv && d.src_layout != PV_SRC_NCTHW && d.src_layout != PV_SRC_NTHWC) return PV_ERR_INVALID;
  if (!yuv && d.src_dtype == PV_U16) return PV_ERR_UNSUPPORTED;   // 16-bit samples are a YUV 4:2:0 source only
  if (d.src_layout == PV_SRC_NTHWC && (d.src_dtype != PV_U8 || d.C != 3)) return PV_ERR_INVALID;
  if (yuv && (!d.yuv2rgb || d.C != 3 || (d.c_step != 1 && d.c_step != 2))) return PV_ERR_INVALID;
  // the dtype / layout matrix
  if (yuv ? (d.src_dtype != PV_U8 && d.src_dtype != PV_U16) : (d.src_dtype != PV_U8 && d.src_dtype != PV_F32)) return PV_ERR_UNSUPPORTED;
  const int sb = d.src_dtype == PV_U16 ? 2 : 1;     // bytes per YUV sample
  if (int e = rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo)) return e;
  // the items and the record behind each of them, as pv_batch_views: only the records the launch's items name are read,
  // a video-major sequence names the record just checked, and the widest column span(s) size the staged rows
  int span = 0, span_c = 0;
  for (int i = 0; i < d.n_items; ++i) {
    const pv_view_item& it = d.items[i];
    if (it.source < 0 || it.source >= d.n_sources || it.row < 0 || it.row >= d.n_rows || it.view < 0 || it.view >= d.n_views)
      return PV_ERR_INVALID;
    const pv_view_source& v = d.sources[it.source];
    if (i == 0 || it.source != d.items[i - 1].source)
      if (int e = fv_check_record(f, v, yuv)) return e;
    rs_widest_span(v.sx, v.x_off, d.n_views, d.Wo, v.Ws, span, span_c);
  }
  FvLaunch g = {};
  const bool inter = d.src_layout == PV_SRC_NTHWC;
  long per_row;                                    // LDS bytes of the two source rows of one output row
  if (yuv) {
    per_row = rs_yuv_pitches(span, span_c, d.c_step, sb, g.pitch, g.pitch_c);
  } else {
    g.pitch = pv_round_up(span * (inter ? 3 : (d.src_dtype == PV_F32 ? 4 : 1)) + 15, 16);
    per_row = 2L * (inter ? 1 : d.C) * g.pitch;
  }
  size_t lds;
  if (int e = rs_strip_rows(per_row, d.Ho, g.R, lds)) return e;
  g.c_base = 2 * g.R * g.pitch;
  if (yuv && sb == 2) {
    return pv_frame_yuv16_launch(&d, g.R, g.pitch, g.pitch_c, g.c_base, lds, stream);   // pv_frames16.hip
  } else if (yuv) {
    if (d.c_step == 2) RS_DISPATCH(frame_yuv_kernel, 2);
    else RS_DISPATCH(frame_yuv_kernel, 1);
  } else if (inter) {
    RS_DISPATCH(frame_views_kernel, unsigned char, true);
  } else if (d.src_dtype == PV_U8) {
    RS_DISPATCH(frame_views_kernel, unsigned char, false);
  } else {
    RS_DISPATCH(frame_views_kernel, float, false);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_frame_views(const pv_frame_views_desc* fp, pv_stream_t stream) {
  if (!fp) return PV_ERR_INVALID;
  return fv_run(*fp, stream);
}
