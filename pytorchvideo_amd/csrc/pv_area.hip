// pv_area_views: pv_batch_views / pv_frame_views with a BOX FILTER in place of the four-tap blend (include/pv_mi355x.h, "box-
// filtered downscale"): every output pixel is the mean of all the source pixels under its window, the windows being those of
// F.interpolate(mode="area").  A 1080p decoder surface scaled to a short side of 256 then reaches the network averaged, not
// point-sampled, and no float RGB copy of the video, no interpolate pass and no crop stand between the decoder and the ingest.
//
// A box filter reads every source row under a strip, not two per output row, so the staged strips of pv_rs.h cannot carry it.
// The body here is a staged TILE (the shape of rs_tile_rgb / rs_tile_yuv, without the orientation map): one workgroup owns R
// output rows x X output columns (blockIdx.x = strip * tiles_x + column tile) of one frame t of one item zi.
//   1. stage: the windows of the tile's outputs cover ONE rectangle of the source, rows [start_y(first), end_y(last)) x columns
//      likewise.  Its rows are copied to LDS in the source dtype exactly as the tiles of pv_rs.h copy theirs: the aligned 16-byte
//      granules that cover each row's span, a batch of four loads per thread, the LDS image of a row keeping the span's
//      `addr & 15`.  YUV stages the chroma rectangle [ys0 >> 1, (ys1 - 1) >> 1] x [xs0 >> 1, (xs1 - 1) >> 1] behind the luma one
//      (4:2:0; the shifts are the layout's, RsSub of pv_rs.h).
//      Tiling in x keeps the staged bytes independent of the frame width (a no-crop view of a 2160p frame is 3840 columns).
//   2. barrier; sum: a thread owns ONE output pixel, so all 256 threads work whatever the destination form.  It walks its
//      window's columns in ascending order and, per column, the window's rows in ascending order (the pinned order: the column
//      sum first, then the sum of the column sums), divides once, applies the affine map and leaves the fp32 result in a second
//      LDS image [c][R][X].  A column sum is needed by the one or two outputs of its row whose windows hold the column, so it
//      is formed where it is used and never shared.  YUV converts and clamps every tap with yuv_tap2 -- two rows of one
//      column per call, the packed-fp32 pair -- before it is added.
//   3. barrier; store: a thread takes G x-adjacent results of one row from that image and hands them to rs_store_group, so the
//      three destination forms, their 16-byte stores and their edge handling are the strips' own.  X is a multiple of 8, so a
//      group starts where a strip's group starts.
// The host sizes R, X, the staged rows and the LDS pitch(es) from the widest footprint over the records x views the launch's
// items name (ar_size), with the very calls the kernel makes; none of them enters a value.  A workgroup whose footprint
// exceeds them -- a device copy that is not the validated one -- stages nothing and writes nothing.
// In front of the body stand the item loader and the geometry builders of pv_rs.h, serving whole videos and frame lists
// (`frames` is workgroup-uniform, as in pv_orient.hip); the body does not read sy / sx: its windows are integers.
// 3 RGB / planar forms and 2 chroma arrangements x 2 sample widths, x 5 destination forms: 35 kernels.
#include "pv_area.h"

namespace {

// ArLaunch, the tile of a workgroup, the store, ar_tile_rgb and ar_tile_yuv are in pv_area.h: pv_packed.hip and pv_yuv4.hip
// instantiate them too.
constexpr int kArTiles[][2] = {{8, 64}, {8, 32}, {4, 32}, {4, 16}, {2, 16}, {2, 8}, {1, 8}};   // R x X, largest first

// S / INTER / FORM / D: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void area_views_kernel(const pv_batch_views_desc d, const ArLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ar_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  ar_tile_rgb<S, INTER, FORM, D>(ar_lds, g, rs_item_rgb(item), item.S->Hn, item.S->Wn, rs_dst(d, d.C), zi, t);
}

// CSTEP / SMP / FORM / D: as rs_strip_yuv.
template <int CSTEP, typename SMP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void area_yuv_kernel(const pv_batch_views_desc d, const ArLaunch g, const int frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ay_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsItem item = rs_item<RS_EITHER>(d, zi, t, frames);
  ar_tile_yuv<CSTEP, FORM, D, SMP>(ay_lds, g, rs_item_yuv<CSTEP>(item), item.S->Hn, item.S->Wn, rs_dst(d, 3), d.yuv2rgb, zi, t);
}

#define AR_TILES(KERNEL, ...) RS_DISPATCH(pv_ceil_div(d.Ho, g.R) * g.tiles_x, lds, (d, g, fr), KERNEL, __VA_ARGS__)
#define AR_RGB(S, INTER) AR_TILES(area_views_kernel, S, INTER)
#define AR_YUV(CSTEP, SMP) AR_TILES(area_yuv_kernel, CSTEP, SMP)

// Folds the widest footprint of an R x X tile of record v over its views into n: source rows, source columns, chroma rows,
// chroma columns.  Rows and columns are independent, so the bands of strips and of column tiles are walked separately, with
// the very calls the kernel makes (ar_tile).
inline void ar_footprint(const pv_view_source& v, int n_views, int Ho, int Wo, int R, int X, int (&n)[4], RsSub sub) {
  auto fold = [&](int lo, int end, int at) {       // source interval [lo, end) of rows (at = 0) / of columns (at = 1)
    const int cs = at == 0 ? sub.csy : sub.csx;    // the chroma shift of the axis
    const int a = end - lo, c = ((end - 1) >> cs) - (lo >> cs) + 1;
    n[at] = a > n[at] ? a : n[at];
    n[at + 2] = c > n[at + 2] ? c : n[at + 2];
  };
  for (int view = 0; view < n_views; ++view) {
    int lo, end, unused;
    for (int row0 = 0; row0 < Ho; row0 += R) {
      rs_area_win(v.y_off[view] + row0, v.Hs, v.Hn, lo, unused);
      rs_area_win(v.y_off[view] + row0 + (R < Ho - row0 ? R : Ho - row0) - 1, v.Hs, v.Hn, unused, end);
      fold(lo, end, 0);
    }
    for (int col0 = 0; col0 < Wo; col0 += X) {
      rs_area_win(v.x_off[view] + col0, v.Ws, v.Wn, lo, unused);
      rs_area_win(v.x_off[view] + col0 + (X < Wo - col0 ? X : Wo - col0) - 1, v.Ws, v.Wn, unused, end);
      fold(lo, end, 1);
    }
  }
}

// R x X, the staged rows and the LDS pitch(es) of a launch over `records` (the records the launch's items name): the largest
// tile of kArTiles whose widest footprint, with the results behind it, fits the staging budget of the strips, else the
// smallest one if it fits the LDS limit.  That last refusal needs a window of some 2000 taps per channel plane (a ratio
// beyond 50 for uint8 sources, beyond 25 for fp32 ones: a 2160p frame scaled to a short side of 80).
inline int ar_size(const pv_batch_views_desc& d, const std::vector<const pv_view_source*>& records, ArLaunch& g, size_t& lds) {
  constexpr size_t n_tiles = sizeof(kArTiles) / sizeof(kArTiles[0]);
  RsSub sub = {1, 1};
  rs_yuv_sub(d.src_layout, &sub);
  for (size_t k = 0; k < n_tiles; ++k) {
    const int R = kArTiles[k][0], X = kArTiles[k][1];
    int n[4] = {0, 0, 0, 0};
    for (const pv_view_source* v : records) ar_footprint(*v, d.n_views, d.Ho, d.Wo, R, X, n, sub);
    g = {};
    g.R = R, g.X = X, g.tiles_x = (int32_t)pv_ceil_div(d.Wo, X);
    long bytes = rs_tile_layout(d, n, g);           // the staged source rectangle, as a tile of pv_rs.h lays it out
    if (bytes > kRsLdsMax) {                       // before it is narrowed to 32 bits
      if (k + 1 == n_tiles) return PV_ERR_UNSUPPORTED;
      continue;
    }
    g.out_base = (int32_t)bytes;                   // pitches are multiples of 16
    bytes += (long)d.C * R * X * (long)sizeof(float);
    lds = (size_t)bytes;
    if (bytes <= kRsLdsBudget) return PV_OK;
    if (k + 1 == n_tiles) return bytes <= kRsLdsMax ? PV_OK : PV_ERR_UNSUPPORTED;
  }
  return PV_ERR_UNSUPPORTED;
}

// The descriptor as the wrapped entry point checks it (rs_check_item_desc), then every item (rs_walk_items): its range and
// its record (rs_check_record with the entry point's check of `src`) -- all of PV_ERR_INVALID first --, then what this entry
// point does not carry: oriented records and products beyond the index limit.  The launch is sized from the records the items
// name.
template <typename CheckSrc>
int ar_run(const pv_batch_views_desc& d, bool frames, const CheckSrc& check_src, pv_stream_t stream) {
  if (int e = rs_check_item_desc(d)) return e;
  const bool yuv = rs_yuv_sub(d.src_layout);
  std::vector<const pv_view_source*> records;      // the records the items name, a video-major run once
  const auto check = [&](const pv_view_source& v) { return rs_check_record(d, v, yuv, check_src); };
  const auto each = [&](const pv_view_item&, const pv_view_source& v, bool again) {
    if (!again) records.push_back(&v);
    return PV_OK;
  };
  if (int e = rs_walk_items(d, check, each)) return e;
  constexpr long kIndexLimit = 1L << 24;
  for (const pv_view_source* v : records) {
    if (v->orient != 0) return PV_ERR_UNSUPPORTED;
    if ((long)v->Hs * v->Hn > kIndexLimit || (long)v->Ws * v->Wn > kIndexLimit) return PV_ERR_UNSUPPORTED;
  }
  ArLaunch g = {};
  size_t lds = 0;
  if (int e = ar_size(d, records, g, lds)) return e;
  if (rs_packed_px(d.src_layout)) return pv_packed_area(d, frames, g, lds, stream);   // pv_packed.hip
  if (rs_yuv4(d.src_layout)) return pv_yuv4_area(d, frames, g, lds, stream);           // pv_yuv4.hip
  if (rs_yuyv(d.src_layout)) return pv_yuyv_area(d, frames, g, lds, stream);           // pv_yuyv.hip
  const int fr = frames ? 1 : 0;
  RS_SOURCE_FORMS(AR_RGB, AR_YUV);
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_area_views(const pv_area_views_desc* ap, pv_stream_t stream) {
  if (!ap) return PV_ERR_INVALID;
  if (ap->filter != PV_FILTER_AREA) return PV_ERR_INVALID;
  if (ap->reserved[0] != 0 || ap->reserved[1] != 0 || ap->reserved[2] != 0) return PV_ERR_INVALID;
  const pv_batch_views_desc& d = ap->frames.batch;
  return fv_with_table(ap->frames, [&](bool frames, const auto& check_src) { return ar_run(d, frames, check_src, stream); });
}
