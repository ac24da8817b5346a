// The kernels of YUV 4:2:2 and 4:4:4 launches (include/pv_mi355x.h, "YUV 4:2:2 and 4:4:4": src_layout PV_SRC_YUV422,
// PV_SRC_YUV444) of pv_batch_views, pv_frame_views, pv_region_views and pv_area_views: what MJPEG cameras (yuvj422p), ProRes /
// DNxHR and contribution feeds (yuv422p10le), capture SDKs (NV16 / P210), screen recordings and High 4:4:4 streams
// (yuv444p, yuv444p10le) decode to, read where it lies instead of through a chroma decimation into a 4:2:0 copy.
//
// Nothing here computes: the bodies are the YUV bodies of the ingest -- rs_strip_yuv and rs_tile_yuv (pv_rs.h), ar_tile_yuv
// (pv_area.h) -- instantiated with RsSub (pv_rs.h), which changes ONE thing of them and no expression of a value: the chroma
// sample of luma pixel (y, x) is (y >> csy, x >> csx) where the 4:2:0 kernels have (y >> 1, x >> 1).  The pair is a kernel
// argument, uniform over the launch and held in scalar registers, so ONE kernel serves 4:2:2 (0, 1) and 4:4:4 (0, 0) of its
// chroma arrangement and sample width; a shift by a scalar register costs what the shift by 1 costs.  What is staged follows
// the same shifts: the chroma span [xs0 >> csx, xs1 >> csx] of chroma rows (y >> csy); a dense strip stages every chroma row
// of its run once, which is up to 2R rows here (R + 1 for 4:2:0) -- the strip's LDS holds 2R chroma slots in either case,
// because the sparse staging needs them.  The taps, the three fused multiply-adds and the clamp per tap, the pinned blend, the
// windows and their summation order, the affine map and the single rounding are the bodies' own, so an item holds, bit for
// bit, what the 4:2:0 launch writes for the frames whose chroma this layout replicates.
//
// In front of the bodies stand the item loader and the geometry builders of pv_rs.h, serving whole videos and frame lists
// (`frames` is workgroup-uniform, as in pv_region.hip and pv_area.hip).  The entry points validate and size (rs_item_launch,
// rg_run, ar_run: chroma rows and columns are counted by the same shifts there) and call the four launch functions below.
// 4 bodies x 2 chroma arrangements x 2 sample widths x 5 destination forms: 80 kernels.
#include "pv_area.h"

namespace {

// CSTEP / SMP / FORM / D: as rs_strip_yuv.  Upright records of pv_batch_views / pv_frame_views: the staged strip.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv4_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                const RsSub c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char y4_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_strip_yuv<CSTEP, FORM, D, SMP>(y4_lds, g.R, g.pitch, g.pitch_c, g.c_base, rs_item_yuv<CSTEP>(item), rs_dst(d, 3), d.yuv2rgb, zi,
                                    t, true, RsTapNone(), c);
}

// Oriented records of the two: the staged tile.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv4_orient_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames,
                                                                 const RsSub c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char o4_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_tile_yuv<CSTEP, FORM, D, SMP>(o4_lds, g, rs_item_yuv<CSTEP>(item), item.orient, rs_dst(d, 3), d.yuv2rgb, zi, t, RsTapNone(), c);
}

// pv_region_views: the staged strip over the rectangle of (row, t), as region_yuv_kernel (pv_region.hip) sets it up.  The
// members the subsampling halves are even (checked on the host: rg_check_region), so chroma row (top + y) >> csy is
// (top >> csy) + (y >> csy), and likewise for columns.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv4_region_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                 const pv_view_region* __restrict__ regions, const RsSub c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char r4_lds[];
  constexpr int SB = (int)sizeof(SMP), CB = CSTEP * SB;
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RgItem item = rg_item(d, regions, frames, zi, t);
  RsYuvSrc s = rs_item_yuv<CSTEP>(item);
  s.Hs = item.h, s.Ws = item.w;
  s.sy = item.sy, s.sx = item.sx;
  s.yoff = 0, s.xoff = 0;
  // the rectangle's origin, folded in: luma into the frame offset, and the chroma planes -- addressed from the same frame
  // offset -- by what their origin differs from it
  const long luma0 = (long)item.top * s.y_pitch + (long)item.left * SB;
  const long chroma0 = (long)(item.top >> c.csy) * s.c_pitch + (long)(item.left >> c.csx) * CB;
  s.frame_off += luma0;
  s.c_off_a += chroma0 - luma0, s.c_off_b += chroma0 - luma0;
  rs_strip_yuv<CSTEP, FORM, D, SMP>(r4_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true, RsTapNone(), c);
}

// pv_area_views: the staged tile of the box filter.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv4_area_kernel(const pv_batch_views_desc d, const ArLaunch g, const int frames,
                                                               const RsSub c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char a4_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  ar_tile_yuv<CSTEP, FORM, D, SMP>(a4_lds, g, rs_item_yuv<CSTEP>(item), item.S->Hn, item.S->Wn, rs_dst(d, 3), d.yuv2rgb, zi, t, c);
}

// The chroma-arrangement and sample-width dispatch in front of the destination-form dispatch; expects d and stream in scope.
#define Y4_LAUNCH(GRID_X, LDS, ARGS, KERNEL)                                         \
  do {                                                                               \
    RsSub c;                                                                         \
    if (!rs_yuv4(d.src_layout) || !rs_yuv_sub(d.src_layout, &c)) return PV_ERR_INVALID; \
    const int fr = frames ? 1 : 0;                                                   \
    if (d.src_dtype == PV_U16) {                                                     \
      if (d.c_step == 2) RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 2, unsigned short);  \
      else RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 1, unsigned short);                \
    } else {                                                                         \
      if (d.c_step == 2) RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 2, unsigned char);   \
      else RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 1, unsigned char);                 \
    }                                                                                \
    PV_LAUNCH_CHECK();                                                               \
    return PV_OK;                                                                    \
  } while (0)

}  // namespace

int pv_yuv4_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0) return PV_ERR_INVALID;             // not sized: no upright item was announced
  Y4_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, c), yuv4_views_kernel);
}

int pv_yuv4_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.TR <= 0 || g.TC <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  Y4_LAUNCH(pv_ceil_div(d.Ho, g.TR) * g.tiles_x, lds, (d, g, fr, c), yuv4_orient_kernel);
}

int pv_yuv4_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                    pv_stream_t stream) {
  if (g.R <= 0 || !regions) return PV_ERR_INVALID;
  Y4_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, regions, c), yuv4_region_kernel);
}

int pv_yuv4_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0 || g.X <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  Y4_LAUNCH(pv_ceil_div(d.Ho, g.R) * g.tiles_x, lds, (d, g, fr, c), yuv4_area_kernel);
}
