// pv_frame_views: pv_batch_views with every FRAME individually addressed.  A hardware decoder hands out surfaces from a pool
// -- one allocation per frame, uniform geometry and pitch, any order, reused -- and a live stream never is one tensor; here
// a source is a slice of a device table of frame base addresses instead of one allocation with a constant frame stride.
//
// The kernels are the staged strips of pv_rs.h (rs_strip_rgb, rs_strip_yuv) behind the item loader and the geometry builders
// of pv_rs.h, as in pv_batch.hip, with the loader told at compile time that sources are frame lists (rs_item<RS_FRAMES>).
// Where batch_views_kernel multiplies the table entry by the frame size, these load the frame's base address from the
// record's slice (record.src + 8 * entry) -- one more workgroup-uniform, scalar load -- and hand the body a geometry with the
// frame at offset 0: a one-frame source (N = 1, ts = 0) for the RGB / planar forms, frame_off = 0 for YUV.  Every other
// value the body sees is the one batch_views_kernel gives it, so an item holds the bits pv_batch_views writes for the same
// frames in one allocation.  The body fetches only the aligned 16-byte granules that cover a byte of the span, and such a
// granule lies in the page of that byte: a frame that ends at the end of its allocation is safe.
//
// What stays per launch -- R, the LDS pitch(es): RsItemLaunch -- is sized as pv_batch_views sizes it, from the host copies of
// the records the items name.  The descriptor embeds a whole pv_batch_views_desc, and one routine validates and sizes both
// (rs_item_launch, pv_rs.h); fv_run checks the pointer table in front of it and hands it the check of a record's `src`,
// read as a table slice.
//
// This file holds two kernel wrappers (frame_views_kernel, frame_yuv_kernel: 25 kernels) and the dispatch over them.  PV_U16
// sources (16-bit YUV samples) are validated and sized here and launched from pv_frames16.hip, which holds their wrapper,
// frame_yuv16_kernel: the two differ in the sample type alone.  The second translation unit stays because the code-object
// tests compile the two apart and count the kernels of each; build time argues neither way (10 s and 5 s of a parallel build
// whose slowest units take 27 s).
#include "pv_frames.h"

namespace {

// S / INTER / FORM / D: as rs_strip_rgb.  One frame is a dense [C, Hs, Ws] (plane stride of ONE frame) or [Hs, Ws, 3].
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void frame_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fv_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsRgbSrc s = rs_item_rgb(rs_item<RS_FRAMES>(d, zi, t));
  rs_strip_rgb<S, INTER, FORM, D>(fv_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, true);
}

// CSTEP / FORM / D: as rs_strip_yuv.  One frame is one surface: the record's offsets and pitches, from the frame's base.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void frame_yuv_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fy_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsYuvSrc s = rs_item_yuv<CSTEP>(rs_item<RS_FRAMES>(d, zi, t));
  rs_strip_yuv<CSTEP, FORM, D>(fy_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

#define FV_RGB(S, INTER) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), frame_views_kernel, S, INTER)
#define FV_YUV(CSTEP, SMP)                                                                          \
  do {                                                                                              \
    if (sizeof(SMP) == 2) return pv_frame_yuv16_launch(d, g, lds, stream);   /* pv_frames16.hip */  \
    RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), frame_yuv_kernel, CSTEP);                      \
  } while (0)

// The pointer table, then rs_item_launch (pv_rs.h) for everything pv_batch_views checks and sizes too.  This entry point's own
// part of a record is its `src`, a slice of the table (fv_check_table, fv_check_src: pv_frames.h).
int fv_run(const pv_frame_views_desc& f, pv_stream_t stream) {
  if (int e = fv_check_table(f)) return e;
  const auto check_src = fv_check_src(f);
  RsItemLaunch g;
  RsTileLaunch tg;
  size_t lds, lds_t;
  if (int e = rs_item_launch(f.batch, check_src, g, lds, tg, lds_t)) return e;
  // the strips of a run of upright items: the whole launch when no record is oriented
  auto upright = [&](const pv_batch_views_desc& d) -> int {
    if (rs_packed_px(d.src_layout)) return pv_packed_strips(d, true, g, lds, stream);   // pv_packed.hip
    if (rs_yuv4(d.src_layout)) return pv_yuv4_strips(d, true, g, lds, stream);           // pv_yuv4.hip
    if (rs_yuyv(d.src_layout)) return pv_yuyv_strips(d, true, g, lds, stream);           // pv_yuyv.hip
    RS_SOURCE_FORMS(FV_RGB, FV_YUV);
    PV_LAUNCH_CHECK();
    return PV_OK;
  };
  auto oriented = [&](const pv_batch_views_desc& d) -> int { return pv_orient_launch(d, true, tg, lds_t, stream); };   // pv_orient.hip
  return rs_item_runs(f.batch, upright, oriented);
}

}  // namespace

extern "C" int pv_frame_views(const pv_frame_views_desc* fp, pv_stream_t stream) {
  if (!fp) return PV_ERR_INVALID;
  return fv_run(*fp, stream);
}
