// pv_batch_views: the resampling ingest with one SOURCE PER DESTINATION ITEM, so that one launch -- hence one forward --
// holds views of as many videos as it takes to fill the deploy batch (a dataset evaluation: thousands of videos with 3 to 30
// views each, every video with a length and a frame size of its own).
//
// The kernels are resample_crop_kernel (pv_resample.hip) and yuv_views_kernel (pv_yuv.hip) with the geometry those take by
// value -- Hs, Ws, Hn, Wn, the window origins, sy / sx, the source address and, for YUV, the plane offsets -- read from the
// item's 96-byte record (pv_view_source) instead: blockIdx.z loads its 16-byte item, clamps source / row / view into range
// and loads the record.  Everything in the record is uniform over the workgroup, so these are scalar loads; the record is
// read field by field through a pointer (a by-value copy indexed at run time would be scratch) and the view is selected,
// not indexed, as in the one-source kernels.  Coordinates, taps, blend, affine map and stores are the shared code of pv_rs.h
// in the same order, so an item holds the bits pv_video_views / pv_yuv_views writes for its video alone.
//
// What stays per LAUNCH is what sizes the workgroup: R output rows per strip and the LDS pitch(es) of a staged row.  The host
// sizes the pitch from the widest column span over every (source an item refers to) x view and R from the LDS budget, as
// rs_run / yuv_run do for one source; neither enters any value.  Each workgroup decides for its own strip whether the source
// rows fit the 2R slots as one contiguous run (an upscaled source) or are staged in pairs (a 720p source), so both kinds
// share a launch.
#include <cstring>

#include "pv_rs.h"

namespace {

struct BvLaunch {
  int32_t R;          // output rows per workgroup
  int32_t pitch;      // LDS bytes per staged (row, plane) -- YUV: per staged luma row; multiple of 16, >= 15 + widest span
  int32_t pitch_c;    // YUV: LDS bytes per staged chroma (row, plane)
  int32_t c_base;     // YUV: LDS offset of the chroma image: 2 R pitch
};

// The item of this workgroup, clamped into range before anything is addressed through it.
struct BvItem {
  const pv_view_source* __restrict__ S;
  int row, view;
};
__device__ __forceinline__ BvItem bv_item(const pv_batch_views_desc& d, int zi) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  BvItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.row = min(max(it->row, 0), d.n_rows - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  return r;
}

// S: source element (unsigned char | float); INTER: frame-interleaved [N,Hs,Ws,3] source; FORM / D: destination.
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_views_kernel(const pv_batch_views_desc d, const BvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bv_lds[];
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int XB = INTER ? 3 : (int)sizeof(S);   // bytes from one source column to the next
  const int tid = threadIdx.x;
  const int R = g.R, pitch = g.pitch;
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const BvItem item = bv_item(d, zi);
  const pv_view_source* __restrict__ V = item.S;
  const int view = item.view;
  const int Hs = V->Hs, Ws = V->Ws, N = V->N;
  const float sy = V->sy, sx = V->sx;
  // selected, not indexed
  const int yoff = view == 0 ? V->y_off[0] : (view == 1 ? V->y_off[1] : V->y_off[2]);
  const int xoff = view == 0 ? V->x_off[0] : (view == 1 ? V->x_off[1] : V->x_off[2]);
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);
  // clamped before any address is formed: a malformed table can never read outside the item's source
  const int ts = min(max(d.t_index[(long)item.row * d.t_stride + t], 0), N - 1);
  const int planes = INTER ? 1 : d.C;

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(sx, xoff, Ws, xs0, unused, lunused);
  rs_coord(sx, xoff + d.Wo - 1, Ws, unused, xs1, lunused);
  rs_coord(sy, yoff + row0, Hs, ybase, unused, lunused);
  rs_coord(sy, yoff + row0 + nrows - 1, Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int span_bytes = (xs1 - xs0 + 1) * XB;
  if (span_bytes + 15 > pitch) return;             // a record the launch was not sized for: nothing is staged or written

  // byte address of column xs0 of source row y of plane `pl` of the selected frame
  const uintptr_t src0 = reinterpret_cast<uintptr_t>(V->src);
  const long row_bytes = (long)Ws * XB;
  const long frame_bytes = (long)Hs * row_bytes;
  const long first = (long)ts * frame_bytes + (long)xs0 * XB;
  const long plane_bytes = INTER ? 0 : (long)N * frame_bytes;
  auto row_addr = [&](int y, int pl) -> uintptr_t { return src0 + first + (long)pl * plane_bytes + (long)y * row_bytes; };

  // ---- stage -------------------------------------------------------------------------------------------------
  const int cpr = pitch >> 4;                      // 16-byte chunks per staged row
  const int total = nslots * planes * cpr;
  for (int base = tid; base < total; base += kRsThreads * 4) {
    u32x4 val[4];
    int off[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * kRsThreads;
      off[u] = -1;
      if (idx < total) {
        const int sp = idx / cpr, ch = idx - sp * cpr;
        const int slot = sp / planes, pl = sp - slot * planes;
        int y = ybase + slot;
        if (!dense) {
          int i0, i1;
          rs_coord(sy, yoff + row0 + (slot >> 1), Hs, i0, i1, lunused);
          y = (slot & 1) ? i1 : i0;
        }
        const uintptr_t a = row_addr(y, pl);
        if (ch * 16 < (int)(a & 15) + span_bytes) {
          val[u] = *reinterpret_cast<const u32x4*>((a & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = sp * pitch + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(bv_lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- gather ------------------------------------------------------------------------------------------------
  float sc[4], sh[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = (d.ch_scale && c < d.C) ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift && c < d.C) ? d.ch_shift[c] : 0.f;
  }
  const int gpr = (d.Wo + G - 1) / G;              // groups per output row
  const int items = nrows * gpr;
  for (int it = tid; it < items; it += kRsThreads) {
    const int r = it / gpr, gx = it - r * gpr;
    const int y = row0 + r;
    int i0y, i1y;
    float ly1;
    rs_coord(sy, yoff + y, Hs, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int s0 = dense ? i0y - ybase : 2 * r, s1 = dense ? i1y - ybase : 2 * r + 1;
    int ro0[4], ro1[4];                            // LDS byte offset of column xs0, channel c, in the two source rows
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (INTER) {
        ro0[c] = s0 * pitch + (int)(row_addr(i0y, 0) & 15) + c;
        ro1[c] = s1 * pitch + (int)(row_addr(i1y, 0) & 15) + c;
      } else {
        const int cc = c < d.C ? c : 0;
        ro0[c] = (s0 * planes + cc) * pitch + (int)(row_addr(i0y, cc) & 15);
        ro1[c] = (s1 * planes + cc) * pitch + (int)(row_addr(i1y, cc) & 15);
      }
    }
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(gx * G + j, d.Wo - 1);     // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(sx, xoff + x, Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = (i0x - xs0) * XB, o1 = (i1x - xs0) * XB;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < d.C) {
          const float p00 = rs_tap<S>(bv_lds, ro0[c] + o0), p01 = rs_tap<S>(bv_lds, ro0[c] + o1);
          const float p10 = rs_tap<S>(bv_lds, ro1[c] + o0), p11 = rs_tap<S>(bv_lds, ro1[c] + o1);
          const float v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
          out[c][j] = v * sc[c] + sh[c];
        } else {
          out[c][j] = 0.f;
        }
      }
    }
    const int x0 = gx * G;
    const int nvalid = min(G, d.Wo - x0);
    rs_store_group<FORM, D, G>(d.dst, out, d.C, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, nvalid);
  }
}

// CSTEP: bytes between x-adjacent samples of one chroma plane (2: U and V interleaved in ONE staged plane; 1: two planes).
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void batch_yuv_kernel(const pv_batch_views_desc d, const BvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char by_lds[];
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int CP = CSTEP == 1 ? 2 : 1;           // staged chroma planes
  const int tid = threadIdx.x;
  const int R = g.R, pitch_y = g.pitch, pitch_c = g.pitch_c;
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const BvItem item = bv_item(d, zi);
  const pv_view_source* __restrict__ V = item.S;
  const int view = item.view;
  const int Hs = V->Hs, Ws = V->Ws;
  const float sy = V->sy, sx = V->sx;
  const int y_pitch = V->y_pitch, c_pitch = V->c_pitch;
  // selected, not indexed
  const int yoff = view == 0 ? V->y_off[0] : (view == 1 ? V->y_off[1] : V->y_off[2]);
  const int xoff = view == 0 ? V->x_off[0] : (view == 1 ? V->x_off[1] : V->x_off[2]);
  // which byte of an interleaved pair is U / V, and where the staged chroma plane(s) start inside a frame: the record's
  const long u_off = V->u_offset, v_off = V->v_offset;
  const long c_min = u_off < v_off ? u_off : v_off;
  const long c_off_a = CSTEP == 2 ? c_min : u_off, c_off_b = CSTEP == 2 ? c_min : v_off;
  const int u_byte = CSTEP == 2 ? (int)(u_off - c_min) : 0, v_byte = CSTEP == 2 ? (int)(v_off - c_min) : 0;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);
  // clamped before any address is formed: a malformed table can never read outside the item's source
  const int ts = min(max(d.t_index[(long)item.row * d.t_stride + t], 0), V->N - 1);

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(sx, xoff, Ws, xs0, unused, lunused);
  rs_coord(sx, xoff + d.Wo - 1, Ws, unused, xs1, lunused);
  rs_coord(sy, yoff + row0, Hs, ybase, unused, lunused);
  rs_coord(sy, yoff + row0 + nrows - 1, Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int cxs0 = xs0 >> 1, cybase = ybase >> 1;
  const int ncslots = dense ? (ylast >> 1) - cybase + 1 : 2 * nrows;   // dense: <= R + 1 <= 2R
  const int span_y = xs1 - xs0 + 1;
  const int span_c = ((xs1 >> 1) - cxs0 + 1) * CSTEP;
  if (span_y + 15 > pitch_y || span_c + 15 > pitch_c) return;   // a record the launch was not sized for

  const uintptr_t frame = reinterpret_cast<uintptr_t>(V->src) + (long)ts * V->frame_stride;
  auto y_addr = [&](int y) -> uintptr_t { return frame + (long)y * y_pitch + xs0; };
  auto c_addr = [&](int cy, int pl) -> uintptr_t {
    return frame + (pl == 0 ? c_off_a : c_off_b) + (long)cy * c_pitch + (long)cxs0 * CSTEP;
  };

  // ---- stage -------------------------------------------------------------------------------------------------
  const int cpr_y = pitch_y >> 4, cpr_c = pitch_c >> 4;   // 16-byte chunks per staged row
  const int total_y = nslots * cpr_y;
  const int total = total_y + ncslots * CP * cpr_c;
  for (int base = tid; base < total; base += kRsThreads * 4) {
    u32x4 val[4];
    int off[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * kRsThreads;
      off[u] = -1;
      if (idx < total) {
        const bool luma = idx < total_y;
        const int j = luma ? idx : idx - total_y;
        const int cpr = luma ? cpr_y : cpr_c;
        const int sp = j / cpr, ch = j - sp * cpr;             // luma: sp = slot; chroma: sp = slot * CP + plane
        const int slot = luma ? sp : sp / CP, pl = luma ? 0 : sp - slot * CP;
        int y = ybase + slot, cy = cybase + slot;
        if (!dense) {
          int i0, i1;
          rs_coord(sy, yoff + row0 + (slot >> 1), Hs, i0, i1, lunused);
          y = (slot & 1) ? i1 : i0;
          cy = y >> 1;
        }
        const uintptr_t a = luma ? y_addr(y) : c_addr(cy, pl);
        if (ch * 16 < (int)(a & 15) + (luma ? span_y : span_c)) {
          val[u] = *reinterpret_cast<const u32x4*>((a & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = (luma ? sp * pitch_y : g.c_base + sp * pitch_c) + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(by_lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- gather ------------------------------------------------------------------------------------------------
  float m[12], sc[3], sh[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = d.yuv2rgb[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sc[c] = d.ch_scale ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift) ? d.ch_shift[c] : 0.f;
  }
  const int gpr = (d.Wo + G - 1) / G;              // groups per output row
  const int items = nrows * gpr;
  for (int it = tid; it < items; it += kRsThreads) {
    const int r = it / gpr, gx = it - r * gpr;
    const int y = row0 + r;
    int i0y, i1y;
    float ly1;
    rs_coord(sy, yoff + y, Hs, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int s0 = dense ? i0y - ybase : 2 * r, s1 = dense ? i1y - ybase : 2 * r + 1;
    const int cs0 = dense ? (i0y >> 1) - cybase : 2 * r, cs1 = dense ? (i1y >> 1) - cybase : 2 * r + 1;
    // LDS byte offset of column xs0 (luma) / cxs0 (U, V) in the two source rows
    const int yo0 = s0 * pitch_y + (int)(y_addr(i0y) & 15), yo1 = s1 * pitch_y + (int)(y_addr(i1y) & 15);
    const int uo0 = g.c_base + cs0 * CP * pitch_c + (int)(c_addr(i0y >> 1, 0) & 15) + u_byte;
    const int uo1 = g.c_base + cs1 * CP * pitch_c + (int)(c_addr(i1y >> 1, 0) & 15) + u_byte;
    const int vo0 = g.c_base + (cs0 * CP + CP - 1) * pitch_c + (int)(c_addr(i0y >> 1, CP - 1) & 15) + v_byte;
    const int vo1 = g.c_base + (cs1 * CP + CP - 1) * pitch_c + (int)(c_addr(i1y >> 1, CP - 1) & 15) + v_byte;
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(gx * G + j, d.Wo - 1);     // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(sx, xoff + x, Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = i0x - xs0, o1 = i1x - xs0;
      const int c0 = ((i0x >> 1) - cxs0) * CSTEP, c1 = ((i1x >> 1) - cxs0) * CSTEP;
      f32x2 p0[3], p1[3];                          // {row i0y, row i1y} of column i0x / i1x, per channel
      yuv_tap2(m, by_lds, yo0 + o0, uo0 + c0, vo0 + c0, yo1 + o0, uo1 + c0, vo1 + c0, p0);
      yuv_tap2(m, by_lds, yo0 + o1, uo0 + c1, vo0 + c1, yo1 + o1, uo1 + c1, vo1 + c1, p1);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][j] = yuv_blend(ly0, ly1, lx0, lx1, p0[c], p1[c], sc[c], sh[c]);
      out[3][j] = 0.f;
      // finish this pixel before the next one starts (see yuv_views_kernel: the register count)
      asm volatile("" : "+v"(out[0][j]), "+v"(out[1][j]), "+v"(out[2][j]));
    }
    const int x0 = gx * G;
    rs_store_group<FORM, D, G>(d.dst, out, 3, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, min(G, d.Wo - x0));
  }
}

#define BV_DISPATCH(KERNEL, ...)                                                                                         \
  do {                                                                                                                   \
    if (d.dst_layout == PV_DST_NCTHW) {                                                                                  \
      if (d.dst_dtype == PV_BF16) PV_LAUNCH((KERNEL<__VA_ARGS__, RS_PLANAR, bf16_t>), grid, block, lds, s, d, g);        \
      else PV_LAUNCH((KERNEL<__VA_ARGS__, RS_PLANAR, float>), grid, block, lds, s, d, g);                                \
    } else if (d.c_p == 4) {                                                                                             \
      PV_LAUNCH((KERNEL<__VA_ARGS__, RS_C4, bf16_t>), grid, block, lds, s, d, g);                                        \
    } else {                                                                                                             \
      if (d.dst_dtype == PV_BF16) PV_LAUNCH((KERNEL<__VA_ARGS__, RS_CL, bf16_t>), grid, block, lds, s, d, g);            \
      else PV_LAUNCH((KERNEL<__VA_ARGS__, RS_CL, float>), grid, block, lds, s, d, g);                                    \
    }                                                                                                                    \
  } while (0)

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// One record of a launch: a source, positive sizes, windows inside the scaled frame, sy / sx the library's own division, and
// for YUV the planes inside a frame.
int bv_check_record(const pv_batch_views_desc& d, const pv_view_source& v, bool yuv) {
  if (!v.src || v.N <= 0 || v.Hs <= 0 || v.Ws <= 0 || v.Hn <= 0 || v.Wn <= 0) return PV_ERR_INVALID;
  if (int e = rs_check_views(d.n_views, v.y_off, v.x_off, d.Ho, d.Wo, v.Hn, v.Wn)) return e;
  if (!same_bits(v.sy, (float)v.Hs / (float)v.Hn) || !same_bits(v.sx, (float)v.Ws / (float)v.Wn)) return PV_ERR_INVALID;
  if (yuv) return rs_check_yuv_planes(v.Hs, v.Ws, d.c_step, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset);
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
  if (d.src_layout == PV_SRC_NTHWC && (d.src_dtype != PV_U8 || d.C != 3)) return PV_ERR_INVALID;
  if (yuv && (!d.yuv2rgb || d.C != 3 || (d.c_step != 1 && d.c_step != 2))) return PV_ERR_INVALID;
  // the dtype / layout matrix
  if (yuv ? d.src_dtype != PV_U8 : (d.src_dtype != PV_U8 && d.src_dtype != PV_F32)) return PV_ERR_UNSUPPORTED;
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
    for (int k = 0; k < d.n_views; ++k) {
      int a, b, u;
      float l;
      rs_coord(v.sx, v.x_off[k], v.Ws, a, u, l);
      rs_coord(v.sx, v.x_off[k] + d.Wo - 1, v.Ws, u, b, l);
      span = b - a + 1 > span ? b - a + 1 : span;
      const int c = (b >> 1) - (a >> 1) + 1;
      span_c = c > span_c ? c : span_c;
    }
  }
  BvLaunch g = {};
  const bool inter = d.src_layout == PV_SRC_NTHWC;
  long per_row;                                    // LDS bytes of the two source rows of one output row
  if (yuv) {
    g.pitch = pv_round_up(span + 15, 16);
    g.pitch_c = pv_round_up(span_c * d.c_step + 15, 16);
    per_row = 2L * (g.pitch + (long)(d.c_step == 2 ? 1 : 2) * g.pitch_c);
  } else {
    g.pitch = pv_round_up(span * (inter ? 3 : (d.src_dtype == PV_F32 ? 4 : 1)) + 15, 16);
    per_row = 2L * (inter ? 1 : d.C) * g.pitch;
  }
  long R = kRsLdsBudget / per_row;
  R = R > kRsMaxRows ? kRsMaxRows : R;
  R = R > d.Ho ? d.Ho : R;
  if (R < 1) R = 1;
  if (R * per_row > kRsLdsMax) return PV_ERR_UNSUPPORTED;
  g.R = (int)R;
  g.c_base = (int32_t)(2 * R * g.pitch);
  const size_t lds = (size_t)(R * per_row);
  const dim3 grid((unsigned)pv_ceil_div(d.Ho, R), (unsigned)d.T, (unsigned)d.n_items), block(kRsThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (yuv) {
    if (d.c_step == 2) BV_DISPATCH(batch_yuv_kernel, 2);
    else BV_DISPATCH(batch_yuv_kernel, 1);
  } else if (inter) {
    BV_DISPATCH(batch_views_kernel, unsigned char, true);
  } else if (d.src_dtype == PV_U8) {
    BV_DISPATCH(batch_views_kernel, unsigned char, false);
  } else {
    BV_DISPATCH(batch_views_kernel, float, false);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

}  // namespace

extern "C" int pv_batch_views(const pv_batch_views_desc* dp, pv_stream_t stream) {
  if (!dp) return PV_ERR_INVALID;
  return bv_run(*dp, stream);
}
