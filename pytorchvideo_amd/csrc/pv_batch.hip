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
// What stays per LAUNCH is what sizes the workgroup (RsItemLaunch): R output rows per strip and the LDS pitch(es) of a staged
// row.  The host sizes the pitch from the widest column span over every (source an item refers to) x view and R from the LDS
// budget, as rs_run / yuv_run do for one source; neither enters any value.  Each workgroup decides for its own strip whether
// the source rows fit the 2R slots as one contiguous run (an upscaled source) or are staged in pairs (a 720p source), so both
// kinds share a launch.  A record whose span exceeds the pitch -- only possible when the device copy is not the validated
// host copy -- makes the body return before it stages anything.
//
// This file holds the three kernel wrappers (batch_views_kernel, batch_yuv_kernel, batch_yuv16_kernel: 35 kernels) and the
// dispatch over them.  The host checks and the sizing are rs_item_launch (pv_rs.h), shared with pv_frame_views; what is
// checked here is only that a record's `src` is one allocation of the source dtype.
#include "pv_rs.h"

namespace {

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
__global__ __launch_bounds__(kRsThreads) void batch_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
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
__global__ __launch_bounds__(kRsThreads) void batch_yuv_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
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
__global__ __launch_bounds__(kRsThreads) void batch_yuv16_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
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

// Validation and sizing are rs_item_launch's (pv_rs.h); this entry point's own part is the record's `src`, one allocation:
// 4-byte aligned for fp32, even for 16-bit samples (either dtype outside its layouts is refused before a record is read).
// Items of oriented records (orient != 0) are not for these kernels: rs_item_runs hands each run of them to the tile kernels.
int bv_run(const pv_batch_views_desc& desc, pv_stream_t stream) {
  RsItemLaunch g;
  RsTileLaunch tg;
  size_t lds, lds_t;
  const auto check_src = rs_check_video_src(desc.src_dtype);
  if (int e = rs_item_launch(desc, check_src, g, lds, tg, lds_t)) return e;
  // the strips of a run of upright items: the whole launch when no record is oriented
  auto upright = [&](const pv_batch_views_desc& d) -> int {
    const bool yuv = d.src_layout == PV_SRC_YUV420;
    if (yuv && d.src_dtype == PV_U16) {
      if (d.c_step == 2) RS_DISPATCH(batch_yuv16_kernel, 2);
      else RS_DISPATCH(batch_yuv16_kernel, 1);
    } else if (yuv) {
      if (d.c_step == 2) RS_DISPATCH(batch_yuv_kernel, 2);
      else RS_DISPATCH(batch_yuv_kernel, 1);
    } else if (d.src_layout == PV_SRC_NTHWC) {
      RS_DISPATCH(batch_views_kernel, unsigned char, true);
    } else if (d.src_dtype == PV_U8) {
      RS_DISPATCH(batch_views_kernel, unsigned char, false);
    } else {
      RS_DISPATCH(batch_views_kernel, float, false);
    }
    PV_LAUNCH_CHECK();
    return PV_OK;
  };
  auto oriented = [&](const pv_batch_views_desc& d) -> int { return pv_orient_launch(d, false, tg, lds_t, stream); };   // pv_orient.hip
  return rs_item_runs(desc, upright, oriented);
}

}  // namespace

extern "C" int pv_batch_views(const pv_batch_views_desc* dp, pv_stream_t stream) {
  if (!dp) return PV_ERR_INVALID;
  return bv_run(*dp, stream);
}
