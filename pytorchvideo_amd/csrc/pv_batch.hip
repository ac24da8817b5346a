// pv_batch_views: the resampling ingest with one SOURCE PER DESTINATION ITEM, so that one launch -- hence one forward --
// holds views of as many videos as it takes to fill the deploy batch (a dataset evaluation: thousands of videos with 3 to 30
// views each, every video with a length and a frame size of its own).
//
// The kernels are the staged strips of pv_rs.h (rs_strip_rgb, rs_strip_yuv), the bodies of pv_video_views / pv_yuv_views,
// with the geometry those take by value -- Hs, Ws, the window origins, sy / sx, the source address and, for YUV, the plane
// offsets -- read from the item's 96-byte record (pv_view_source) instead: rs_item loads and clamps the item of blockIdx.z,
// rs_item_rgb / rs_item_yuv fill the geometry from its record (pv_rs.h; pv_frame_views and the entry points built on the
// two use the same pair).  One body serves both, so an item holds the bits pv_video_views / pv_yuv_views writes for its video
// alone.
//
// What stays per LAUNCH is what sizes the workgroup (RsItemLaunch): R output rows per strip and the LDS pitch(es) of a staged
// row.  The host sizes the pitch from the widest column span over every (source an item refers to) x view and R from the LDS
// budget, as rs_run / yuv_run do for one source; neither enters any value.  Each workgroup decides for its own strip whether
// the source rows fit the 2R slots as one contiguous run (an upscaled source) or are staged in pairs (a 720p source), so both
// kinds share a launch.  A record whose span exceeds the pitch -- only possible when the device copy is not the validated
// host copy -- makes the body return before it stages anything.
//
// This file holds the three kernel wrappers (batch_views_kernel, batch_yuv_kernel, batch_yuv16_kernel: 35 kernels) and the
// dispatch over them.  The 8-bit and the 16-bit YUV wrapper differ in the sample type alone and keep a name each: the
// code-object tests count the kernels of each name.  The host checks and the sizing are rs_item_launch (pv_rs.h), shared with
// pv_frame_views; what is checked here is only that a record's `src` is one allocation of the source dtype.
#include "pv_rs.h"

namespace {

// S / INTER / FORM / D: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsRgbSrc s = rs_item_rgb(rs_item<RS_VIDEOS>(d, zi, t));
  rs_strip_rgb<S, INTER, FORM, D>(bv_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, true);
}

// CSTEP / FORM / D: as rs_strip_yuv.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_yuv_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char by_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsYuvSrc s = rs_item_yuv<CSTEP>(rs_item<RS_VIDEOS>(d, zi, t));
  rs_strip_yuv<CSTEP, FORM, D>(by_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

// The same on two-byte samples (PV_U16 / pv_yuv16_views).
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_yuv16_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char by_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsYuvSrc s = rs_item_yuv<CSTEP>(rs_item<RS_VIDEOS>(d, zi, t));
  rs_strip_yuv<CSTEP, FORM, D, unsigned short>(by_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

#define BV_STRIPS(KERNEL, ...) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), KERNEL, __VA_ARGS__)
#define BV_RGB(S, INTER) BV_STRIPS(batch_views_kernel, S, INTER)
#define BV_YUV(CSTEP, SMP)                                             \
  do {                                                                 \
    if (sizeof(SMP) == 2) BV_STRIPS(batch_yuv16_kernel, CSTEP);        \
    else BV_STRIPS(batch_yuv_kernel, CSTEP);                           \
  } while (0)

// Validation and sizing are rs_item_launch's (pv_rs.h); this entry point's own part is the record's `src`, one allocation:
// 4-byte aligned for fp32, even for 16-bit samples (either dtype outside its layouts is refused before a record is read).
// Items of oriented records (orient != 0) are not for these kernels: rs_item_runs hands each run of them to the tile kernels.
int bv_run(const pv_batch_views_desc& desc, pv_stream_t stream) {
  RsItemLaunch g;
  RsTileLaunch tg;
  size_t lds, lds_t;
  const auto check_src = rs_check_video_src(desc.src_dtype, desc.src_layout);
  if (int e = rs_item_launch(desc, check_src, g, lds, tg, lds_t)) return e;
  // the strips of a run of upright items: the whole launch when no record is oriented
  auto upright = [&](const pv_batch_views_desc& d) -> int {
    if (rs_packed_px(d.src_layout)) return pv_packed_strips(d, false, g, lds, stream);   // pv_packed.hip
    if (rs_yuv4(d.src_layout)) return pv_yuv4_strips(d, false, g, lds, stream);           // pv_yuv4.hip
    if (rs_yuyv(d.src_layout)) return pv_yuyv_strips(d, false, g, lds, stream);           // pv_yuyv.hip
    RS_SOURCE_FORMS(BV_RGB, BV_YUV);
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
