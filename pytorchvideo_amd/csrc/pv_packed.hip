// The kernels of PACKED-PIXEL launches (include/pv_mi355x.h, "packed pixels": src_layout PV_SRC_BGR, PV_SRC_RGBA, PV_SRC_BGRA,
// PV_SRC_ARGB, PV_SRC_ABGR) of pv_batch_views, pv_frame_views, pv_region_views and pv_area_views: what an OpenCV pipeline holds
// (BGR24) and what screen capture, colour converters and compositor surfaces hand out (32-bit pixels, usually pitched), read
// where they lie instead of through a channel-select pass over the whole video.
//
// Nothing here computes: the bodies are the RGB bodies of the ingest -- rs_strip_rgb and rs_tile_rgb (pv_rs.h), ar_tile_rgb
// (pv_area.h) -- instantiated with RsPacked<PB> (pv_rs.h), which changes three things of them and no expression of a value:
//   a column is PB = 3 or 4 bytes;
//   rows lie at the record's y_pitch and frames at its frame_stride, as the YUV bodies address luma rows;
//   R, G and B are bytes o[0..2] of a pixel.  The offsets are a kernel argument, uniform over the launch and held in scalar
//   registers, so ONE kernel serves every channel order of its pixel size: two source forms (PB 3, PB 4), not five.
//   PB == 4 reads a tap as one dword from LDS and takes the channels out of the register (v_bfe_u32 with a scalar offset);
//   PB == 3 reads bytes, as the [.., 3] form does.
// The taps, the pinned coordinate, the blend, the windows and their summation order, the affine map and the single rounding are
// the bodies' own, so an item holds, bit for bit, what the same entry point writes with PV_SRC_NTHWC for the dense R, G, B copy
// of the same frames.  The fourth byte of a pixel and the bytes between Ws * PB and the pitch are staged with the granules that
// hold them and never read from LDS.
//
// In front of the bodies stand the item loader and the geometry builders of pv_rs.h, serving whole videos and frame lists
// (`frames` is workgroup-uniform, as in pv_region.hip and pv_area.hip).  The entry points validate and size (rs_item_launch,
// rg_run, ar_run: a column counts PB bytes there) and call the four launch functions below.
// 4 bodies x 2 pixel sizes x 5 destination forms: 40 kernels.
#include "pv_area.h"

namespace {

// PB / FORM / D: the pixel size and the destination.  Upright records of pv_batch_views / pv_frame_views: the staged strip.
template <int PB, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void packed_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                  const RsPackedArg o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pk_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_strip_rgb<unsigned char, true, FORM, D>(pk_lds, g.R, g.pitch, rs_item_rgb(item), rs_dst(d, 3), zi, t, true,
                                             rs_item_packed<PB>(item.S, o));
}

// Oriented records of the two: the staged tile.
template <int PB, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void packed_orient_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames,
                                                                   const RsPackedArg o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char po_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  rs_tile_rgb<unsigned char, true, FORM, D>(po_lds, g, rs_item_rgb(item), item.orient, rs_dst(d, 3), zi, t,
                                            rs_item_packed<PB>(item.S, o));
}

// pv_region_views: the staged strip over the rectangle of (row, t).
template <int PB, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void packed_region_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                   const pv_view_region* __restrict__ regions, const RsPackedArg o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pr_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RgItem item = rg_item(d, regions, frames, zi, t);
  rs_strip_rgb<unsigned char, true, FORM, D>(pr_lds, g.R, g.pitch, rg_item_rgb(item), rs_dst(d, 3), zi, t, true,
                                             rs_item_packed<PB>(item.S, o));
}

// pv_area_views: the staged tile of the box filter.
template <int PB, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void packed_area_kernel(const pv_batch_views_desc d, const ArLaunch g, const int frames,
                                                                 const RsPackedArg o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pa_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  ar_tile_rgb<unsigned char, true, FORM, D>(pa_lds, g, rs_item_rgb(item), item.S->Hn, item.S->Wn, rs_dst(d, 3), zi, t,
                                            rs_item_packed<PB>(item.S, o));
}

// The pixel-size dispatch in front of the destination-form dispatch; expects d and stream in scope.
#define PK_LAUNCH(GRID_X, LDS, ARGS, KERNEL)                               \
  do {                                                                     \
    RsPackedArg o;                                                         \
    const int pb = rs_packed_px(d.src_layout, &o);                         \
    if (pb == 0) return PV_ERR_INVALID;                                    \
    const int fr = frames ? 1 : 0;                                         \
    if (pb == 4) RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 4);                \
    else RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, 3);                        \
    PV_LAUNCH_CHECK();                                                     \
    return PV_OK;                                                          \
  } while (0)

}  // namespace

int pv_packed_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0) return PV_ERR_INVALID;             // not sized: no upright item was announced
  PK_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, o), packed_views_kernel);
}

int pv_packed_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.TR <= 0 || g.TC <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  PK_LAUNCH(pv_ceil_div(d.Ho, g.TR) * g.tiles_x, lds, (d, g, fr, o), packed_orient_kernel);
}

int pv_packed_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                      pv_stream_t stream) {
  if (g.R <= 0 || !regions) return PV_ERR_INVALID;
  PK_LAUNCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, regions, o), packed_region_kernel);
}

int pv_packed_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream) {
  if (g.R <= 0 || g.X <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;
  PK_LAUNCH(pv_ceil_div(d.Ho, g.R) * g.tiles_x, lds, (d, g, fr, o), packed_area_kernel);
}
