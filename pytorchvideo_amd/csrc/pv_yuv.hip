// pv_yuv_views: pv_video_views on decoder-native YUV 4:2:0 frames (NV12 / NV21: one interleaved chroma plane, c_step 2;
// I420 / YV12: two chroma planes, c_step 1).  The arithmetic is pinned in include/pv_mi355x.h: every TAP is converted to
// RGB in registers (three fused multiply-adds per channel, clamped to [0, 255]), then blended, mapped and stored as
// pv_resample_crop does.  No RGB frame exists anywhere.
//
// The structure is resample_crop_kernel's (pv_resample.hip): one workgroup owns a strip of R output rows of one destination
// frame of one view.
//   1. stage: the luma span of the source rows the strip needs (per output row i0y, i1y; or, when those rows are at most 2R,
//      that contiguous run once) and the chroma span behind it -- chroma rows (y >> 1) of the same rows, columns
//      [xs0 >> 1, xs1 >> 1]; in the contiguous case every chroma row once, so half as many as luma rows -- are copied to LDS
//      with aligned 16-byte global loads and 16-byte LDS writes.  Rows start at any byte address (a pitched surface, an odd
//      base, the +1 of the second interleaved sample): the loads fetch the aligned granules that cover the span and the LDS
//      image keeps the span's offset inside its first granule (`addr & 15`).  A granule that covers a byte of a span lies in
//      the same page as that byte, so the up to 15 bytes in front of and behind it are never used and never fault.
//   2. gather: a thread owns G x-adjacent output pixels of one row, takes the four Y taps and the (U, V) pair behind each of
//      them from LDS, converts, clamps, blends in fp32, applies the affine map and hands the group to rs_store_group.
#include "pv_rs.h"

namespace {

struct YuvLaunch {
  float sy, sx;          // (float)Hs / (float)Hn, (float)Ws / (float)Wn: divided once, on the host
  int32_t R;             // output rows per workgroup
  int32_t pitch_y;       // LDS bytes per staged luma row: multiple of 16, >= 15 + widest span
  int32_t pitch_c;       // LDS bytes per staged chroma (row, plane)
  int32_t c_base;        // LDS offset of the chroma image: 2 R pitch_y
  int32_t u_byte, v_byte;   // c_step 2: which byte of an interleaved pair is U / V; c_step 1: 0
  int64_t c_off_a, c_off_b; // byte offset inside a frame of staged chroma plane 0 / 1 (c_step 2: only plane 0, min(u, v))
};

// CSTEP: bytes between x-adjacent samples of one chroma plane (2: U and V interleaved in ONE staged plane; 1: two planes).
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void yuv_views_kernel(const pv_yuv_views_desc d, const YuvLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char yv_lds[];
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int CP = CSTEP == 1 ? 2 : 1;           // staged chroma planes
  const int tid = threadIdx.x;
  const int R = g.R, pitch_y = g.pitch_y, pitch_c = g.pitch_c;
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const int item = d.item0 + zi;
  const int clip = item / d.n_views, view = item - clip * d.n_views;
  // selected, not indexed: a runtime index into the by-value descriptor would put it in scratch
  const int yoff = view == 0 ? d.y_off[0] : (view == 1 ? d.y_off[1] : d.y_off[2]);
  const int xoff = view == 0 ? d.x_off[0] : (view == 1 ? d.x_off[1] : d.x_off[2]);
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);
  // clamped before any address is formed: a malformed table can never read outside the source
  const int ts = min(max(d.t_index[(long)clip * d.t_stride + t], 0), d.N - 1);

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(g.sx, xoff, d.Ws, xs0, unused, lunused);
  rs_coord(g.sx, xoff + d.Wo - 1, d.Ws, unused, xs1, lunused);
  rs_coord(g.sy, yoff + row0, d.Hs, ybase, unused, lunused);
  rs_coord(g.sy, yoff + row0 + nrows - 1, d.Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int cxs0 = xs0 >> 1, cybase = ybase >> 1;
  const int ncslots = dense ? (ylast >> 1) - cybase + 1 : 2 * nrows;   // dense: <= R + 1 <= 2R
  const int span_y = xs1 - xs0 + 1;
  const int span_c = ((xs1 >> 1) - cxs0 + 1) * CSTEP;

  const uintptr_t frame = reinterpret_cast<uintptr_t>(d.src) + (long)ts * d.frame_stride;
  auto y_addr = [&](int y) -> uintptr_t { return frame + (long)y * d.y_pitch + xs0; };
  auto c_addr = [&](int cy, int pl) -> uintptr_t {
    return frame + (pl == 0 ? g.c_off_a : g.c_off_b) + (long)cy * d.c_pitch + (long)cxs0 * CSTEP;
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
          rs_coord(g.sy, yoff + row0 + (slot >> 1), d.Hs, i0, i1, lunused);
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
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(yv_lds + off[u]) = val[u];
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
    rs_coord(g.sy, yoff + y, d.Hs, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int s0 = dense ? i0y - ybase : 2 * r, s1 = dense ? i1y - ybase : 2 * r + 1;
    const int cs0 = dense ? (i0y >> 1) - cybase : 2 * r, cs1 = dense ? (i1y >> 1) - cybase : 2 * r + 1;
    // LDS byte offset of column xs0 (luma) / cxs0 (U, V) in the two source rows
    const int yo0 = s0 * pitch_y + (int)(y_addr(i0y) & 15), yo1 = s1 * pitch_y + (int)(y_addr(i1y) & 15);
    const int uo0 = g.c_base + cs0 * CP * pitch_c + (int)(c_addr(i0y >> 1, 0) & 15) + g.u_byte;
    const int uo1 = g.c_base + cs1 * CP * pitch_c + (int)(c_addr(i1y >> 1, 0) & 15) + g.u_byte;
    const int vo0 = g.c_base + (cs0 * CP + CP - 1) * pitch_c + (int)(c_addr(i0y >> 1, CP - 1) & 15) + g.v_byte;
    const int vo1 = g.c_base + (cs1 * CP + CP - 1) * pitch_c + (int)(c_addr(i1y >> 1, CP - 1) & 15) + g.v_byte;
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(gx * G + j, d.Wo - 1);     // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(g.sx, xoff + x, d.Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = i0x - xs0, o1 = i1x - xs0;
      const int c0 = ((i0x >> 1) - cxs0) * CSTEP, c1 = ((i1x >> 1) - cxs0) * CSTEP;
      f32x2 p0[3], p1[3];                          // {row i0y, row i1y} of column i0x / i1x, per channel
      yuv_tap2(m, yv_lds, yo0 + o0, uo0 + c0, vo0 + c0, yo1 + o0, uo1 + c0, vo1 + c0, p0);
      yuv_tap2(m, yv_lds, yo0 + o1, uo0 + c1, vo0 + c1, yo1 + o1, uo1 + c1, vo1 + c1, p1);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][j] = yuv_blend(ly0, ly1, lx0, lx1, p0[c], p1[c], sc[c], sh[c]);
      out[3][j] = 0.f;
      // finish this pixel before the next one starts: left alone, the compiler blends all G pixels together at the end and
      // keeps every converted tap alive until then (170+ VGPRs for G = 8: two waves per SIMD)
      asm volatile("" : "+v"(out[0][j]), "+v"(out[1][j]), "+v"(out[2][j]));
    }
    const int x0 = gx * G;
    rs_store_group<FORM, D, G>(d.dst, out, 3, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, min(G, d.Wo - x0));
  }
}

template <int CSTEP>
int yuv_launch(const pv_yuv_views_desc& d, const YuvLaunch& g, dim3 grid, size_t lds, hipStream_t s) {
  const dim3 block(kRsThreads);
  if (d.dst_layout == PV_DST_NCTHW) {
    if (d.dst_dtype == PV_BF16) PV_LAUNCH((yuv_views_kernel<CSTEP, RS_PLANAR, bf16_t>), grid, block, lds, s, d, g);
    else PV_LAUNCH((yuv_views_kernel<CSTEP, RS_PLANAR, float>), grid, block, lds, s, d, g);
  } else if (d.c_p == 4) {
    PV_LAUNCH((yuv_views_kernel<CSTEP, RS_C4, bf16_t>), grid, block, lds, s, d, g);
  } else {
    if (d.dst_dtype == PV_BF16) PV_LAUNCH((yuv_views_kernel<CSTEP, RS_CL, bf16_t>), grid, block, lds, s, d, g);
    else PV_LAUNCH((yuv_views_kernel<CSTEP, RS_CL, float>), grid, block, lds, s, d, g);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

int yuv_run(pv_yuv_views_desc d, pv_stream_t stream) {
  if (d.n_clips <= 0 || d.T <= 0 || d.N <= 0 || d.Hs <= 0 || d.Ws <= 0 || d.Hn <= 0 || d.Wn <= 0 || d.Ho <= 0 || d.Wo <= 0)
    return PV_ERR_INVALID;
  if (d.t_stride < d.T) return PV_ERR_INVALID;
  if (int e = rs_check_yuv_planes(d.Hs, d.Ws, d.c_step, d.y_pitch, d.c_pitch, d.frame_stride, d.u_offset, d.v_offset)) return e;
  if (int e = rs_check_views(d.n_views, d.y_off, d.x_off, d.Ho, d.Wo, d.Hn, d.Wn)) return e;
  if (int e = rs_check_items(d.item0, d.n_items, (long)d.n_clips * d.n_views, d.T)) return e;
  if (int e = rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo)) return e;

  YuvLaunch g;
  g.sy = (float)d.Hs / (float)d.Hn;
  g.sx = (float)d.Ws / (float)d.Wn;
  const bool inter = d.c_step == 2;
  const int64_t c_min = d.u_offset < d.v_offset ? d.u_offset : d.v_offset;
  g.c_off_a = inter ? c_min : d.u_offset;
  g.c_off_b = inter ? c_min : d.v_offset;
  g.u_byte = inter ? (int32_t)(d.u_offset - c_min) : 0;
  g.v_byte = inter ? (int32_t)(d.v_offset - c_min) : 0;
  // the widest luma and chroma column spans of any view size the staged rows
  int span_y = 0, span_c = 0;
  for (int v = 0; v < d.n_views; ++v) {
    int a, b, u;
    float l;
    rs_coord(g.sx, d.x_off[v], d.Ws, a, u, l);
    rs_coord(g.sx, d.x_off[v] + d.Wo - 1, d.Ws, u, b, l);
    span_y = b - a + 1 > span_y ? b - a + 1 : span_y;
    const int c = (b >> 1) - (a >> 1) + 1;
    span_c = c > span_c ? c : span_c;
  }
  g.pitch_y = pv_round_up(span_y + 15, 16);
  g.pitch_c = pv_round_up(span_c * d.c_step + 15, 16);
  const int planes = inter ? 1 : 2;
  const long per_row = 2L * (g.pitch_y + (long)planes * g.pitch_c);   // two source rows per output row, each with its chroma
  long R = kRsLdsBudget / per_row;
  R = R > kRsMaxRows ? kRsMaxRows : R;
  R = R > d.Ho ? d.Ho : R;
  if (R < 1) R = 1;
  if (R * per_row > kRsLdsMax) return PV_ERR_UNSUPPORTED;
  g.R = (int)R;
  g.c_base = (int32_t)(2 * R * g.pitch_y);
  const size_t lds = (size_t)(R * per_row);
  const dim3 grid((unsigned)pv_ceil_div(d.Ho, R), (unsigned)d.T, (unsigned)d.n_items);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return inter ? yuv_launch<2>(d, g, grid, lds, s) : yuv_launch<1>(d, g, grid, lds, s);
}

}  // namespace

extern "C" int pv_yuv_views(const pv_yuv_views_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->src || !dp->dst || !dp->t_index || !dp->yuv2rgb) return PV_ERR_INVALID;
  return yuv_run(*dp, stream);
}
