// pv_resample_crop: short_side_scale + uniform_crop (reference transforms/functional.py:92-131,302-347) fused with the
// ingest's frame selection, Div255 + Normalize affine, dtype conversion and layout change.
// pv_video_views: the same kernel reading ONE video through a frame table with a row per clip -- the clip sampler,
// FrameVideo.get_clip (data/frame_video.py:149-200) and UniformTemporalSubsample of the reference's data pipeline as data.
//
// A bandwidth-bound gather.  One workgroup owns a strip of R output rows of one destination frame of one view:
//   1. stage: the source span those rows need -- per output row the two source rows i0y, i1y (or, when the strip's source
//      rows are fewer than 2R, as in upscaling, that contiguous run of rows once), columns [i0x(first), i1x(last)] -- is
//      copied to LDS in the SOURCE dtype with aligned 16-byte global loads and 16-byte LDS writes.  A row of the span may
//      start at any byte address (Ws = 340 gives 4-byte-aligned rows, an odd Ws none at all): the loads fetch the aligned
//      16-byte granules that cover the span, and the LDS image of each row keeps the span's offset inside its first
//      granule (`addr & 15`), so unaligned rows cost nothing extra.  A granule that covers a byte of the span lies in the
//      same page as that byte, so the up to 15 bytes fetched in front of and behind the span are never used and never fault.
//   2. gather: a thread owns G x-adjacent output pixels of one row (G = one 16-byte store per channel row for planar
//      destinations, 2 = one 16-byte chunk for the 4-channel layout, 1 voxel for channels-last), takes its 4 taps per
//      channel from LDS, blends in fp32, applies the affine map and stores 16-byte chunks.  Groups cut by the right edge
//      (Wo not a multiple of G) or not 16-byte aligned in the destination (odd Wo) are stored element by element.
//      (Eight pixels per thread for the 4-channel layout -- four 16-byte stores 64 bytes apart, as ingest_c4_vec8_kernel
//      does -- measured up to 17 % slower here: DESIGN.md 4.6.)
#include "pv_rs.h"

namespace {

struct RsLaunch {
  float sy, sx;     // (float)Hs / (float)Hn, (float)Ws / (float)Wn: divided once, on the host
  int32_t R;        // output rows per workgroup
  int32_t pitch;    // LDS bytes per staged (row, plane): multiple of 16, >= 15 + widest span
  int32_t src_T;    // frames per source plane; every selected frame is clamped into [0, src_T - 1]
  int32_t item0;
  int32_t tab_stride;   // t_index row stride per clip: 0 = one row shared by all clips (pv_resample_crop)
  int64_t clip_frames;  // frames from one source clip to the next: 0 = every clip reads the one video (pv_video_views)
};

// S: source element (unsigned char | float); INTER: frame-interleaved [B,T,Hs,Ws,3] source; FORM / D: destination.
// Source clip b starts g.clip_frames frames behind clip b - 1 and takes its frames from row b * g.tab_stride of d.t_index:
// B clips with one shared row (pv_resample_crop), or one video with a row per clip (pv_video_views: clip_frames == 0).
template <typename S, bool INTER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void resample_crop_kernel(const pv_resample_desc d, const RsLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int XB = INTER ? 3 : (int)sizeof(S);   // bytes from one source column to the next
  const int tid = threadIdx.x;
  const int R = g.R, pitch = g.pitch;
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const int item = g.item0 + zi;
  const int b = item / d.n_views, view = item - b * d.n_views;
  // selected, not indexed: a runtime index into the by-value descriptor would put it in scratch
  const int yoff = view == 0 ? d.y_off[0] : (view == 1 ? d.y_off[1] : d.y_off[2]);
  const int xoff = view == 0 ? d.x_off[0] : (view == 1 ? d.x_off[1] : d.x_off[2]);
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);
  // clamped before any address is formed: a malformed table can never read outside the source
  const int ts = min(max(d.t_index ? d.t_index[(long)b * g.tab_stride + t] : t, 0), g.src_T - 1);
  const int planes = INTER ? 1 : d.C;

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(g.sx, xoff, d.Ws, xs0, unused, lunused);
  rs_coord(g.sx, xoff + d.Wo - 1, d.Ws, unused, xs1, lunused);
  rs_coord(g.sy, yoff + row0, d.Hs, ybase, unused, lunused);
  rs_coord(g.sy, yoff + row0 + nrows - 1, d.Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int span_bytes = (xs1 - xs0 + 1) * XB;

  // byte address of column xs0 of source row y of plane `pl` of the selected frame
  const uintptr_t src0 = reinterpret_cast<uintptr_t>(d.src);
  const long row_bytes = (long)d.Ws * XB;
  const long frame_bytes = (long)d.Hs * row_bytes;
  const long first = ((long)b * g.clip_frames + ts) * frame_bytes + (long)xs0 * XB;
  const long plane_bytes = INTER ? 0 : (long)g.src_T * frame_bytes;
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
          rs_coord(g.sy, yoff + row0 + (slot >> 1), d.Hs, i0, i1, lunused);
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
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(rs_lds + off[u]) = val[u];
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
    rs_coord(g.sy, yoff + y, d.Hs, i0y, i1y, ly1);
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
      rs_coord(g.sx, xoff + x, d.Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = (i0x - xs0) * XB, o1 = (i1x - xs0) * XB;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < d.C) {
          const float p00 = rs_tap<S>(rs_lds, ro0[c] + o0), p01 = rs_tap<S>(rs_lds, ro0[c] + o1);
          const float p10 = rs_tap<S>(rs_lds, ro1[c] + o0), p11 = rs_tap<S>(rs_lds, ro1[c] + o1);
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

template <typename S, bool INTER>
int rs_launch(const pv_resample_desc& d, const RsLaunch& g, dim3 grid, size_t lds, hipStream_t s) {
  const dim3 block(kRsThreads);
  if (d.dst_layout == PV_DST_NCTHW) {
    if (d.dst_dtype == PV_BF16) PV_LAUNCH((resample_crop_kernel<S, INTER, RS_PLANAR, bf16_t>), grid, block, lds, s, d, g);
    else PV_LAUNCH((resample_crop_kernel<S, INTER, RS_PLANAR, float>), grid, block, lds, s, d, g);
  } else if (d.c_p == 4) {
    PV_LAUNCH((resample_crop_kernel<S, INTER, RS_C4, bf16_t>), grid, block, lds, s, d, g);
  } else {
    if (d.dst_dtype == PV_BF16) PV_LAUNCH((resample_crop_kernel<S, INTER, RS_CL, bf16_t>), grid, block, lds, s, d, g);
    else PV_LAUNCH((resample_crop_kernel<S, INTER, RS_CL, float>), grid, block, lds, s, d, g);
  }
  PV_LAUNCH_CHECK();
  return PV_OK;
}

// Validation and launch shared by both entry points.  `one_video`: the source is one video [C,src_T,Hs,Ws] / [src_T,Hs,Ws,3]
// every clip reads through its own row of t_index (row stride tab_stride); else B clips and one shared t_index row.
int rs_run(pv_resample_desc d, bool one_video, int tab_stride, pv_stream_t stream) {
  if (d.B <= 0 || d.C <= 0 || d.T <= 0 || d.Hs <= 0 || d.Ws <= 0 || d.Hn <= 0 || d.Wn <= 0 || d.Ho <= 0 || d.Wo <= 0)
    return PV_ERR_INVALID;
  if (d.C > 4) return PV_ERR_INVALID;
  if (int e = rs_check_views(d.n_views, d.y_off, d.x_off, d.Ho, d.Wo, d.Hn, d.Wn)) return e;
  if (d.src_layout != PV_SRC_NCTHW && d.src_layout != PV_SRC_NTHWC) return PV_ERR_INVALID;
  if (d.src_layout == PV_SRC_NTHWC && (d.src_dtype != PV_U8 || d.C != 3)) return PV_ERR_INVALID;
  if (d.t_index && d.src_T <= 0) return PV_ERR_INVALID;
  if (one_video && (!d.t_index || tab_stride < d.T)) return PV_ERR_INVALID;
  if (int e = rs_check_items(d.item0, d.n_items, (long)d.B * d.n_views, d.T)) return e;
  // the dtype / layout matrix
  if (d.src_dtype != PV_U8 && d.src_dtype != PV_F32) return PV_ERR_UNSUPPORTED;
  if (int e = rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo)) return e;
  if (d.src_dtype == PV_F32 && reinterpret_cast<uintptr_t>(d.src) % 4) return PV_ERR_INVALID;

  RsLaunch g;
  g.sy = (float)d.Hs / (float)d.Hn;
  g.sx = (float)d.Ws / (float)d.Wn;
  g.src_T = d.t_index ? d.src_T : d.T;
  g.item0 = d.item0;
  g.tab_stride = one_video ? tab_stride : 0;
  g.clip_frames = one_video ? 0 : (int64_t)(d.src_layout == PV_SRC_NTHWC ? 1 : d.C) * g.src_T;
  // the widest column span of any view sizes the staged row
  const bool inter = d.src_layout == PV_SRC_NTHWC;
  const int xb = inter ? 3 : (d.src_dtype == PV_F32 ? 4 : 1);
  int span = 0;
  for (int v = 0; v < d.n_views; ++v) {
    int a, b, u;
    float l;
    rs_coord(g.sx, d.x_off[v], d.Ws, a, u, l);
    rs_coord(g.sx, d.x_off[v] + d.Wo - 1, d.Ws, u, b, l);
    span = b - a + 1 > span ? b - a + 1 : span;
  }
  g.pitch = pv_round_up(span * xb + 15, 16);
  const int planes = inter ? 1 : d.C;
  const long per_row = 2L * planes * g.pitch;      // two source rows per output row
  long R = kRsLdsBudget / per_row;
  R = R > kRsMaxRows ? kRsMaxRows : R;
  R = R > d.Ho ? d.Ho : R;
  if (R < 1) R = 1;
  if (R * per_row > kRsLdsMax) return PV_ERR_UNSUPPORTED;
  g.R = (int)R;
  const size_t lds = (size_t)(R * per_row);
  const dim3 grid((unsigned)pv_ceil_div(d.Ho, R), (unsigned)d.T, (unsigned)d.n_items);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (inter) return rs_launch<unsigned char, true>(d, g, grid, lds, s);
  if (d.src_dtype == PV_U8) return rs_launch<unsigned char, false>(d, g, grid, lds, s);
  return rs_launch<float, false>(d, g, grid, lds, s);
}

}  // namespace

extern "C" int pv_resample_crop(const pv_resample_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->src || !dp->dst) return PV_ERR_INVALID;
  return rs_run(*dp, false, 0, stream);
}

// One video, one frame table: the same kernel with B = n_clips, src_T = N and a table row per clip.
extern "C" int pv_video_views(const pv_video_views_desc* vp, pv_stream_t stream) {
  if (!vp || !vp->src || !vp->dst) return PV_ERR_INVALID;   // n_clips, T, N, the table and its stride: rs_run (B, T, src_T)
  pv_resample_desc d = {};
  d.src = vp->src; d.dst = vp->dst;
  d.B = vp->n_clips; d.C = vp->C; d.T = vp->T;
  d.src_T = vp->N; d.Hs = vp->Hs; d.Ws = vp->Ws;
  d.src_dtype = vp->src_dtype; d.src_layout = vp->src_layout;
  d.Hn = vp->Hn; d.Wn = vp->Wn; d.Ho = vp->Ho; d.Wo = vp->Wo;
  d.n_views = vp->n_views;
  for (int v = 0; v < 3; ++v) { d.y_off[v] = vp->y_off[v]; d.x_off[v] = vp->x_off[v]; }
  d.item0 = vp->item0; d.n_items = vp->n_items;
  d.dst_layout = vp->dst_layout; d.dst_dtype = vp->dst_dtype;
  d.c_p = vp->c_p; d.ld = vp->ld; d.bs = vp->bs;
  d.t_index = vp->t_index; d.ch_scale = vp->ch_scale; d.ch_shift = vp->ch_shift;
  return rs_run(d, true, vp->t_stride, stream);
}
