// The kernels of packed YUV 4:2:2 launches (include/pv_mi355x.h, "packed YUV 4:2:2": src_layout PV_SRC_YUYV422) of
// pv_batch_views, pv_frame_views, pv_region_views and pv_area_views: what UVC webcams and V4L2 (YUY2), SDI / HDMI capture cards
// (UYVY) and the 10- to 16-bit 4:2:2 surfaces of DXVA / VAAPI / Media Foundation (Y210 / Y212 / Y216) hand out, read where it
// lies instead of through a de-interleave pass into planes.
//
// Nothing here computes: the bodies are the YUV bodies of the ingest -- rs_strip_yuv and rs_tile_yuv (pv_rs.h), ar_tile_yuv
// (pv_area.h) -- instantiated with the macropixel arrangement RsMacro (pv_rs.h), which changes where a sample is fetched from
// and no expression of a value: a source row is ONE run of macropixels of four samples, staged once, and a tap takes its luma,
// U and V from that one staged row at the bytes the record names (u_offset / v_offset inside a macropixel, luma at the other
// two samples).  The subsampling is 4:2:2's, the constant pair RsSub422; CSTEP is 4, the samples between two U samples.  The
// taps, the three fused multiply-adds and the clamp per tap, the pinned blend, the windows and their summation order, the
// affine map and the single rounding are the bodies' own, so an item holds, bit for bit, what the PV_SRC_YUV422 launch writes
// for the de-interleaved planes of the same frames.
//
// In front of the bodies stand the item loader and the geometry builders of pv_rs.h, as in pv_yuv4.hip.  The sample order is
// the record's, workgroup-uniform and in scalar registers: records of YUY2, YVYU, UYVY and VYUY frames share a launch and a
// kernel.  4 bodies x 2 sample widths x 5 destination forms: 40 kernels.
#include "pv_area.h"

namespace {

// The geometry of a body from an item's record: ONE plane, so no chroma plane offsets; u_byte / v_byte are the record's
// offsets inside a macropixel, kept below its 4 SB bytes whatever the device copy of the record holds.
template <int SB> __device__ __forceinline__ RsYuvSrc yuyv_item(const RsItem& item) {
  RsYuvSrc s = rs_item_yuv<1>(item);
  s.u_byte = (int)s.c_off_a & (4 * SB - 1), s.v_byte = (int)s.c_off_b & (4 * SB - 1);
  s.c_off_a = 0, s.c_off_b = 0;
  return s;
}

// SMP / FORM / D: as rs_strip_yuv.  Upright records of pv_batch_views / pv_frame_views: the staged strip.
template <typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuyv_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char yp_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_strip_yuv<4, FORM, D, SMP, RsTapNone, RsSub422, RsMacro>(yp_lds, g.R, g.pitch, g.pitch_c, g.c_base, yuyv_item<sizeof(SMP)>(item),
                                                              rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

// Oriented records of the two: the staged tile.
template <typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuyv_orient_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char op_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_tile_yuv<4, FORM, D, SMP, RsTapNone, RsSub422, RsMacro>(op_lds, g, yuyv_item<sizeof(SMP)>(item), item.orient, rs_dst(d, 3),
                                                             d.yuv2rgb, zi, t);
}

// pv_region_views: the staged strip over the rectangle of (row, t), as region_yuv_kernel (pv_region.hip) sets it up.  left is
// even (checked on the host: rg_check_region), so the rectangle starts at a macropixel: its origin is folded into the frame
// offset, and column x of it is column x of a frame that starts there.
template <typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuyv_region_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                 const pv_view_region* __restrict__ regions) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
  constexpr int SB = (int)sizeof(SMP);
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RgItem item = rg_item(d, regions, frames, zi, t);
  RsYuvSrc s = yuyv_item<SB>(item);
  s.Hs = item.h, s.Ws = item.w;
  s.sy = item.sy, s.sx = item.sx;
  s.yoff = 0, s.xoff = 0;
  s.frame_off += (long)item.top * s.y_pitch + (long)(item.left >> 1) * 4 * SB;
  rs_strip_yuv<4, FORM, D, SMP, RsTapNone, RsSub422, RsMacro>(rp_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi,
                                                              t, true);
}

// pv_area_views: the staged tile of the box filter.
template <typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuyv_area_kernel(const pv_batch_views_desc d, const ArLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ap_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  ar_tile_yuv<4, FORM, D, SMP, RsSub422, RsMacro>(ap_lds, g, yuyv_item<sizeof(SMP)>(item), item.S->Hn, item.S->Wn, rs_dst(d, 3),
                                                  d.yuv2rgb, zi, t);
}

// The sample-width dispatch in front of the destination-form dispatch; expects d and stream in scope.
#define YP_LAUNCH(GRID_X, LDS, ARGS, KERNEL)                                   \
  do {                                                                         \
    if (!rs_yuyv(d.src_layout) || d.c_step != 4) return PV_ERR_INVALID;        \
    const int fr = frames ? 1 : 0;                                             \
    if (d.src_dtype == PV_U16) RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, unsigned short); \
    else RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, unsigned char);                \
    PV_LAUNCH_CHECK();                                                         \
    return PV_OK;                                                              \
  } while (0)

}  // namespace

int pv_yuyv_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0) return PV_ERR_INVALID;             // not sized: no upright item was announced
  YP_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr), yuyv_views_kernel);
}

int pv_yuyv_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.TR <= 0 || g.TC <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  YP_LAUNCH(pv_ceil_div(d.Ho, g.TR) * g.tiles_x, lds, (d, g, fr), yuyv_orient_kernel);
}

int pv_yuyv_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                    pv_stream_t stream) {
  if (g.R <= 0 || !regions) return PV_ERR_INVALID;
  YP_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, regions), yuyv_region_kernel);
}

int pv_yuyv_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0 || g.X <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  YP_LAUNCH(pv_ceil_div(d.Ho, g.R) * g.tiles_x, lds, (d, g, fr), yuyv_area_kernel);
}
