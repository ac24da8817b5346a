// pv_region_views: pv_batch_views / pv_frame_views with a RECTANGLE OF THE FRAME PER DESTINATION FRAME as the source of every
// item (include/pv_mi355x.h, "a rectangle per frame"): an actor tube -- the box a tracker follows through the clip -- is cut
// out and resized to the network's input inside the ingest launch, from the video where it lies.
//
// The kernels are the staged strips of pv_rs.h (rs_strip_rgb, rs_strip_yuv) once more.  A workgroup owns one strip of one
// frame t of one item; its geometry, workgroup-uniform and read with scalar loads, comes from the item's record (the stored
// frame: Hs, Ws, pitches, plane offsets, the source address) AND from the 32-byte region record of (row, t): the rectangle,
// clamped into the stored frame before any address is formed, and sy / sx.  The body then sees the rectangle as its whole
// source -- Hs x Ws = h x w, window origin 0 -- so the pinned coordinate clamps every tap into the rectangle:
//   YUV:           the rectangle's origin is folded into the addresses (frame_off, the chroma plane offsets); its members are
//                  even, so chroma row (top + y) >> 1 is (top >> 1) + (y >> 1), and rs_strip_yuv runs unchanged.
//   RGB / planar:  rs_strip_rgb derives its row and frame strides from the extent it clamps with; RsRgbWin (pv_rs.h) carries
//                  the stored frame's extent and the origin beside the rectangle's, behind a template parameter whose default
//                  leaves every other kernel of the ingest with the instructions it had.
// Hence an item's frame holds the bits pv_batch_views writes for a dense copy of the rectangle with Hn = Ho, Wn = Wo.
//
// The item loader of pv_rs.h serves whole videos and frame lists (`frames` is workgroup-uniform, as in pv_area.hip), and the
// geometry is the builders' with what the rectangle changes written over it.  The launch is sized
// as rs_item_launch sizes one: the pitch from the widest rectangle over the launch's items x T frames, read from the host copy
// of the regions, R from the LDS budget; a workgroup whose span exceeds the pitch -- a device copy that is not the validated
// one -- stages nothing and writes nothing.  Each strip decides dense / sparse staging for itself; a tube is usually
// upscaled, which is the dense case.  3 RGB / planar forms and 2 chroma arrangements x 2 sample widths, x 5 destination
// forms: 35 kernels.
#include "pv_frames.h"

namespace {

// The item with its rectangle is rg_item (pv_rs.h: the packed kernels of pv_packed.hip load it too).
// S / INTER / FORM / D: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void region_views_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                  const pv_view_region* __restrict__ regions) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsRgbWin s = rg_item_rgb(rg_item(d, regions, frames, zi, t));
  rs_strip_rgb<S, INTER, FORM, D>(rg_lds, g.R, g.pitch, s, rs_dst(d, d.C), zi, t, true);
}

// CSTEP / FORM / D / SMP: as rs_strip_yuv.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void region_yuv_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                                const pv_view_region* __restrict__ regions) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ry_lds[];
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
  const long chroma0 = (long)(item.top >> 1) * s.c_pitch + (long)(item.left >> 1) * CB;
  s.frame_off += luma0;
  s.c_off_a += chroma0 - luma0, s.c_off_b += chroma0 - luma0;
  rs_strip_yuv<CSTEP, FORM, D, SMP>(ry_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

#define RG_STRIPS(KERNEL, ...) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g, fr, regions), KERNEL, __VA_ARGS__)
#define RG_RGB(S, INTER) RG_STRIPS(region_views_kernel, S, INTER)
#define RG_YUV(CSTEP, SMP) RG_STRIPS(region_yuv_kernel, CSTEP, SMP)

// One rectangle against the frame of the item's source and the launch's window.
// even: the members a YUV layout's subsampling halves (bit 0: top and h, bit 1: left and w) must be even.
inline int rg_check_region(const pv_view_region& r, const pv_view_source& v, int Ho, int Wo, int even) {
  if (r.h < 1 || r.w < 1 || r.top < 0 || r.left < 0) return PV_ERR_INVALID;
  if ((long)r.top + r.h > v.Hs || (long)r.left + r.w > v.Ws) return PV_ERR_INVALID;
  if (!rs_same_bits(r.sy, (float)r.h / (float)Ho) || !rs_same_bits(r.sx, (float)r.w / (float)Wo)) return PV_ERR_INVALID;
  if (r.reserved[0] != 0 || r.reserved[1] != 0) return PV_ERR_INVALID;
  if ((((even & 1) ? (r.top | r.h) : 0) | ((even & 2) ? (r.left | r.w) : 0)) & 1) return PV_ERR_INVALID;
  return PV_OK;
}

// The descriptor as the wrapped entry point checks it (rs_check_item_desc), one view, then every item (rs_walk_items): its
// range, the stored frames of its record (rs_check_record_frames with the entry point's check of `src`; the record's view
// geometry is not read) and the rectangles of its row against that record.  The widest column span over every (item, t) --
// computed with the very calls the kernel makes -- sizes the staged rows; R and the LDS bytes follow as in rs_item_launch
// (rs_strip_size).
template <typename CheckSrc>
int rg_run(const pv_region_views_desc& r, bool frames, const CheckSrc& check_src, pv_stream_t stream) {
  const pv_batch_views_desc& d = r.frames.batch;
  if (int e = rs_check_item_desc(d)) return e;
  if (d.n_views != 1) return PV_ERR_INVALID;       // so the walk accepts view 0 only
  RsSub sub = {1, 1};
  const bool yuv = rs_yuv_sub(d.src_layout, &sub);
  const int even = yuv ? sub.csy | (sub.csx << 1) : 0;
  int span = 0, span_c = 0;
  bool oriented = false;
  const int32_t origin = 0;
  const auto check = [&](const pv_view_source& v) { return rs_check_record_frames(d, v, yuv, check_src); };
  const auto each = [&](const pv_view_item& it, const pv_view_source& v, bool) -> int {
    oriented |= v.orient != 0;
    const pv_view_region* row = r.regions + (long)it.row * d.t_stride;
    for (int t = 0; t < d.T; ++t) {
      if (int e = rg_check_region(row[t], v, d.Ho, d.Wo, even)) return e;
      rs_widest_span(row[t].sx, &origin, 1, d.Wo, row[t].w, span, span_c, sub.csx);
    }
    return PV_OK;
  };
  if (int e = rs_walk_items(d, check, each)) return e;
  if (oriented) return PV_ERR_UNSUPPORTED;
  RsItemLaunch g = {};
  size_t lds = 0;
  if (int e = rs_strip_size(d, span, span_c, g, lds)) return e;
  if (rs_packed_px(d.src_layout)) return pv_packed_regions(d, frames, g, lds, r.regions_dev, stream);   // pv_packed.hip
  if (rs_yuv4(d.src_layout)) return pv_yuv4_regions(d, frames, g, lds, r.regions_dev, stream);           // pv_yuv4.hip
  if (rs_yuyv(d.src_layout)) return pv_yuyv_regions(d, frames, g, lds, r.regions_dev, stream);           // pv_yuyv.hip
  const int fr = frames ? 1 : 0;
  const pv_view_region* regions = r.regions_dev;
  RS_SOURCE_FORMS(RG_RGB, RG_YUV);
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_region_views(const pv_region_views_desc* rp, pv_stream_t stream) {
  if (!rp) return PV_ERR_INVALID;
  if (!rp->regions || !rp->regions_dev || reinterpret_cast<uintptr_t>(rp->regions_dev) % 4) return PV_ERR_INVALID;
  return fv_with_table(rp->frames, [&](bool frames, const auto& check_src) { return rg_run(*rp, frames, check_src, stream); });
}
