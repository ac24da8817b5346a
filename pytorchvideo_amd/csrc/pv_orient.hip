// The kernels of oriented records (pv_view_source.orient != 0: a video stored turned and / or mirrored, include/pv_mi355x.h)
// of pv_batch_views and pv_frame_views: the staged tiles of pv_rs.h (rs_tile_rgb, rs_tile_yuv).  blockIdx.z loads its item and
// the item's record as rs_item (pv_rs.h) does; the frame is then `src` plus the entry times the frame size (pv_batch_views) or,
// `frames` set, the entry of the record's slice of the pointer table (pv_frame_views) -- a workgroup-uniform choice, so one set
// of 35 kernels serves both entry points.  blockIdx.x is the tile, row-major over the window.  The two entry points validate
// and size (rs_item_launch, rs_tile_size) and call pv_orient_launch for every run of oriented items; upright items never come
// here, and a record whose orient is 0 on the device only would still be written correctly (the map of code 0 is the identity).
//
// The loader and the two fills below are this file's own, not rs_item / rs_item_rgb / rs_item_yuv: they make the choice
// between the two kinds of source with selects after one conditional load, where rs_item branches once.  Behind the shared
// loader all 35 kernels come out with other code -- a shorter prologue, but another register allocation throughout, up to 4
// VGPRs fewer in six of the YUV kernels and up to 4 more in four (profiles/r24/isa_vs_parent.md) -- and a change of that
// size is not taken without measuring it on the device.
#include "pv_rs.h"

namespace {

struct OvItem {
  const pv_view_source* __restrict__ S;
  int view, ts, orient;
  uintptr_t frame;      // frames: the base address of the selected frame
};
__device__ __forceinline__ OvItem ov_item(const pv_batch_views_desc& d, int frames, int zi, int t) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  OvItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  const int row = min(max(it->row, 0), d.n_rows - 1);
  r.ts = min(max(d.t_index[(long)row * d.t_stride + t], 0), r.S->N - 1);
  r.orient = r.S->orient & 7;
  r.frame = 0;
  if (frames) {   // read as constant memory: one scalar load (rs_item, pv_rs.h)
    typedef const uint64_t __attribute__((address_space(4))) * table_ptr;
    r.frame = (uintptr_t) reinterpret_cast<table_ptr>(reinterpret_cast<uintptr_t>(r.S->src))[r.ts];
  }
  return r;
}

// S / INTER / FORM / D: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void orient_views_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ov_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const OvItem item = ov_item(d, frames, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsRgbSrc s;
  s.src = frames ? item.frame : reinterpret_cast<uintptr_t>(V->src);
  s.Hs = V->Hs, s.Ws = V->Ws, s.N = frames ? 1 : V->N;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.ts = frames ? 0 : item.ts;
  s.clip_frame0 = 0;
  rs_tile_rgb<S, INTER, FORM, D>(ov_lds, g, s, item.orient, rs_dst(d, d.C), zi, t);
}

// CSTEP / FORM / D / SMP: as rs_strip_yuv.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void orient_yuv_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char oy_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const OvItem item = ov_item(d, frames, zi, t);
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = frames ? item.frame : reinterpret_cast<uintptr_t>(V->src);
  s.frame_off = frames ? 0 : (long)item.ts * V->frame_stride;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  rs_tile_yuv<CSTEP, FORM, D, SMP>(oy_lds, g, s, item.orient, rs_dst(d, 3), d.yuv2rgb, zi, t);
}

#define OV_TILES(KERNEL, ...) RS_DISPATCH(pv_ceil_div(d.Ho, g.TR) * g.tiles_x, lds, (d, g, fr), KERNEL, __VA_ARGS__)
#define OV_RGB(S, INTER) OV_TILES(orient_views_kernel, S, INTER)
#define OV_YUV(CSTEP, SMP) OV_TILES(orient_yuv_kernel, CSTEP, SMP)

}  // namespace

int pv_orient_launch(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream) {
  const int fr = frames ? 1 : 0;
  if (g.TR <= 0 || g.TC <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;   // not sized: no oriented item was announced
  if (rs_packed_px(d.src_layout)) return pv_packed_tiles(d, frames, g, lds, stream);   // pv_packed.hip
  if (rs_yuv4(d.src_layout)) return pv_yuv4_tiles(d, frames, g, lds, stream);           // pv_yuv4.hip
  if (rs_yuyv(d.src_layout)) return pv_yuyv_tiles(d, frames, g, lds, stream);           // pv_yuyv.hip
  RS_SOURCE_FORMS(OV_RGB, OV_YUV);
  PV_LAUNCH_CHECK();
  return PV_OK;
}
