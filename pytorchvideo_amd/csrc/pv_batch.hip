// pv_batch_views: the resampling ingest with one SOURCE PER DESTINATION ITEM, so that one launch -- hence one forward --
// holds views of as many videos as it takes to fill the deploy batch (a dataset evaluation: thousands of videos with 3 to 30
// views each, every video with a length and a frame size of its own).
//
// The kernels are the staged strips of pv_rs.h (rs_strip_rgb, rs_strip_yuv), the bodies of pv_video_views / pv_yuv_views,
// with the geometry those take by value -- Hs, Ws, the window origins, sy / sx, the source address and, for YUV, the plane
// offsets -- read from the item's 96-byte record (pv_view_source) instead: blockIdx.z loads its 16-byte item, clamps source /
// row / view into range and loads the record.  Everything in the record is uniform over the workgroup, so these are scalar
// loads; the record is read field by field through a pointer (a by-value copy indexed at run time would be scratch) and
// the view is selected, not indexed.  One body serves both, so an item holds the bits pv_video_views / pv_yuv_views writes
// for its video alone.
//
// What stays per LAUNCH is what sizes the workgroup: R output rows per strip and the LDS pitch(es) of a staged row.  The host
// sizes the pitch from the widest column span over every (source an item refers to) x view and R from the LDS budget, as
// rs_run / yuv_run do for one source; neither enters any value.  Each workgroup decides for its own strip whether the source
// rows fit the 2R slots as one contiguous run (an upscaled source) or are staged in pairs (a 720p source), so both kinds
// share a launch.  A record whose span exceeds the pitch -- only possible when the device copy is not the validated host
// copy -- makes the body return before it stages anything.
#include <cstring>

#include "pv_rs.h"

namespace {

struct BvLaunch {
  int32_t R;          // output rows per workgroup
  int32_t pitch;      // LDS bytes per staged (row, plane) -- YUV: per staged luma row; multiple of 16, >= 15 + widest span
  int32_t pitch_c;    // YUV: LDS bytes per staged chroma (row, plane)
  int32_t c_base;     // YUV: LDS offset of the chroma image: 2 R pitch
};

// The item of this workgroup, clamped into range before anything is addressed through it, and the frame its table row
// selects, clamped the same way: a malformed table can never read outside the item's source.
struct BvItem {
  const pv_view_source* __restrict__ S;
  int view, ts;
};
__device__ __forceinline__ BvItem bv_item(const pv_batch_views_desc& d, int zi, int t) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  BvItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  const int row = min(max(it->row, 0), d.n_rows - 1);
  r.ts = min(max(d.t_index[(long)row * d.t_stride + t], 0), r.S->N - 1);
  return r;
}

// S / INTER / FORM / D: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_views_kernel(const pv_batch_views_desc d, const BvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const BvItem item = bv_item(d, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsRgbSrc s;
  s.src = reinterpret_cast<uintptr_t>(V->src);
  s.Hs = V->Hs, s.Ws = V->Ws, s.N = V->N;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.ts = item.ts;
  s.clip_frame0 = 0;
  rs_strip_rgb<S, INTER, FORM, D>(bv_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, true);
}

// CSTEP / FORM / D: as rs_strip_yuv.  Which byte of an interleaved pair is U / V, and where the staged chroma plane(s) start
// inside a frame, follow from the record's offsets.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_yuv_kernel(const pv_batch_views_desc d, const BvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char by_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const BvItem item = bv_item(d, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = reinterpret_cast<uintptr_t>(V->src);
  s.frame_off = (long)item.ts * V->frame_stride;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  rs_strip_yuv<CSTEP, FORM, D>(by_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

// The same on two-byte samples (PV_U16 / pv_yuv16_views).  A kernel of its own, spelled out rather than sharing a wrapper
// with the one above: routed through a common inline function the 8-bit kernels come out with other instructions than
// they had (commuted scalar adds), and their code is pinned.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_yuv16_kernel(const pv_batch_views_desc d, const BvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char by_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const BvItem item = bv_item(d, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = reinterpret_cast<uintptr_t>(V->src);
  s.frame_off = (long)item.ts * V->frame_stride;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  rs_strip_yuv<CSTEP, FORM, D, unsigned short>(by_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// One record of a launch: a source, positive sizes, windows inside the scaled frame, sy / sx the library's own division, and
// for YUV the planes inside a frame.
int bv_check_record(const pv_batch_views_desc& d, const pv_view_source& v, bool yuv) {
  if (!v.src || v.N <= 0 || v.Hs <= 0 || v.Ws <= 0 || v.Hn <= 0 || v.Wn <= 0) return PV_ERR_INVALID;
  if (int e = rs_check_views(d.n_views, v.y_off, v.x_off, d.Ho, d.Wo, v.Hn, v.Wn)) return e;
  if (!same_bits(v.sy, (float)v.Hs / (float)v.Hn) || !same_bits(v.sx, (float)v.Ws / (float)v.Wn)) return PV_ERR_INVALID;
  if (yuv) {
    const int sb = d.src_dtype == PV_U16 ? 2 : 1;
    if (int e = rs_check_yuv_planes(v.Hs, v.Ws, d.c_step, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset, sb)) return e;
    return sb == 2 ? rs_check_yuv16_even(reinterpret_cast<uintptr_t>(v.src), v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset)
                   : PV_OK;
  }
  if (d.src_dtype == PV_F32 && reinterpret_cast<uintptr_t>(v.src) % 4) return PV_ERR_INVALID;
  return PV_OK;
}

int bv_run(const pv_batch_views_desc& d, pv_stream_t stream) {
  if (!d.sources || !d.sources_dev || !d.items || !d.items_dev || !d.t_index || !d.dst) return PV_ERR_INVALID;
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
  // the items, the record behind each of them -- a launch is a window of a longer sequence and reads only the records its
  // items name (the kernel clamps `source` into range and the items are the validated ones), so the cost of a launch does
  // not grow with the number of videos of the whole sequence; a record named again is checked again, which is cheaper than
  // remembering -- and the widest column span(s) of any such record x view, which size the staged rows
  int span = 0, span_c = 0;
  for (int i = 0; i < d.n_items; ++i) {
    const pv_view_item& it = d.items[i];
    if (it.source < 0 || it.source >= d.n_sources || it.row < 0 || it.row >= d.n_rows || it.view < 0 || it.view >= d.n_views)
      return PV_ERR_INVALID;
    const pv_view_source& v = d.sources[it.source];
    if (i == 0 || it.source != d.items[i - 1].source)   // a video-major sequence names the record just checked
      if (int e = bv_check_record(d, v, yuv)) return e;
    rs_widest_span(v.sx, v.x_off, d.n_views, d.Wo, v.Ws, span, span_c);
  }
  BvLaunch g = {};
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
    if (d.c_step == 2) RS_DISPATCH(batch_yuv16_kernel, 2);
    else RS_DISPATCH(batch_yuv16_kernel, 1);
  } else if (yuv) {
    if (d.c_step == 2) RS_DISPATCH(batch_yuv_kernel, 2);
    else RS_DISPATCH(batch_yuv_kernel, 1);
  } else if (inter) {
    RS_DISPATCH(batch_views_kernel, unsigned char, true);
  } else if (d.src_dtype == PV_U8) {
    RS_DISPATCH(batch_views_kernel, unsigned char, false);
  } else {
    RS_DISPATCH(batch_views_kernel, float, false);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_batch_views(const pv_batch_views_desc* dp, pv_stream_t stream) {
  if (!dp) return PV_ERR_INVALID;
  return bv_run(*dp, stream);
}
