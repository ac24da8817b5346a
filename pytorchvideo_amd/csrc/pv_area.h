// The staged-tile bodies of pv_area_views (pv_area.hip describes the three steps), with what they are made of: the launch
// record, the tile of a workgroup and the store of its results.  They are here, not in pv_area.hip, because other translation
// units instantiate them: ar_tile_rgb serves pv_area.hip (the dense forms) and pv_packed.hip (packed pixels: RsPacked,
// pv_rs.h), ar_tile_yuv serves pv_area.hip (4:2:0), pv_yuv4.hip (4:2:2 / 4:4:4: RsSub, pv_rs.h) and pv_yuyv.hip (packed 4:2:2: RsMacro).  The sizing and the entry
// point stay in pv_area.hip.
#pragma once
#include "pv_frames.h"

// What stays per launch: filled by ar_size (pv_area.hip).  It crosses translation units (pv_packed_area), so it has external
// linkage, as RsItemLaunch has.
struct ArLaunch {
  int32_t R, X;             // output rows x columns per workgroup; X a multiple of 8
  int32_t tiles_x;          // column tiles per window row
  int32_t rows, pitch;      // staged source rows, LDS bytes per staged (row, plane) -- YUV: luma
  int32_t rows_c, pitch_c, c_base;   // YUV: staged chroma rows, LDS bytes per chroma (row, plane), LDS offset of the chroma image
  int32_t out_base;         // LDS offset of the fp32 results [c][R][X]; a multiple of 16
};

// The packed-pixel kernels of pv_area_views (pv_packed.hip) on a launch ar_run (pv_area.hip) has validated and sized.
int pv_packed_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream);
// Likewise the YUV 4:2:2 / 4:4:4 kernels of pv_area_views (pv_yuv4.hip).
int pv_yuv4_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream);
// Likewise the packed YUV 4:2:2 kernels of pv_area_views (pv_yuyv.hip).
int pv_yuyv_area(const pv_batch_views_desc& d, bool frames, const ArLaunch& g, size_t lds, pv_stream_t stream);

namespace {

// The tile of this workgroup and the source rectangle under it.
struct ArTile {
  int row0, col0, nrows, ncols;
  int ys0, ys1, xs0, xs1;   // source rows [ys0, ys1) x columns [xs0, xs1)
};
__device__ __forceinline__ ArTile ar_tile(const ArLaunch& g, int Ho, int Wo, int yoff, int xoff, int Hs, int Ws, int Hn, int Wn) {
  ArTile a;
  const int strip = blockIdx.x / g.tiles_x, tile_x = blockIdx.x - strip * g.tiles_x;
  a.row0 = strip * g.R, a.col0 = tile_x * g.X;
  a.nrows = min(g.R, Ho - a.row0), a.ncols = min(g.X, Wo - a.col0);
  int unused;
  rs_area_win(yoff + a.row0, Hs, Hn, a.ys0, unused);
  rs_area_win(yoff + a.row0 + a.nrows - 1, Hs, Hn, unused, a.ys1);
  rs_area_win(xoff + a.col0, Ws, Wn, a.xs0, unused);
  rs_area_win(xoff + a.col0 + a.ncols - 1, Ws, Wn, unused, a.xs1);
  return a;
}

// Step 3: the results of the tile, G x-adjacent pixels of one row per thread, to the destination.
template <int FORM, typename D>
__device__ __forceinline__ void ar_store(const float* res, const ArLaunch& g, const ArTile& a, const RsDst& d, int C, int zi, int t) {
  constexpr int G = RsGroup<FORM, D>::G;
  const int gpr = (a.ncols + G - 1) / G;           // groups per tile row
  const int items = a.nrows * gpr;
  for (int it = threadIdx.x; it < items; it += kRsThreads) {
    const int r = it / gpr, gx = it - r * gpr;
    float out[4][G];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < G; ++j) out[c][j] = c < C ? res[(c * g.R + r) * g.X + gx * G + j] : 0.f;   // past ncols: not stored
    const int x0 = a.col0 + gx * G;
    rs_store_group<FORM, D, G>(d.dst, out, C, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, a.row0 + r, x0, min(G, d.Wo - x0));
  }
}

// S / INTER / FORM / D / PK: as rs_strip_rgb.  Hn x Wn: the scaled frame the windows are counted in.
template <typename S, bool INTER, int FORM, typename D, typename PK = RsDense>
__device__ __forceinline__ void ar_tile_rgb(unsigned char* lds, const ArLaunch& g, const RsRgbSrc& s, int Hn, int Wn, const RsDst& d,
                                            int zi, int t, const PK& pk = PK()) {
  constexpr int XB = PK::kPacked ? PK::PB : (INTER ? 3 : (int)sizeof(S));   // bytes from one source column to the next
  const int tid = threadIdx.x;
  const ArTile a = ar_tile(g, d.Ho, d.Wo, s.yoff, s.xoff, s.Hs, s.Ws, Hn, Wn);
  if (a.nrows <= 0 || a.ncols <= 0) return;
  const int planes = INTER ? 1 : d.C;
  const int pitch = g.pitch;
  const int nslots = a.ys1 - a.ys0;
  const int span_bytes = (a.xs1 - a.xs0) * XB;
  if (nslots > g.rows || span_bytes + 15 > pitch) return;

  // byte address of column xs0 of source row y of plane `pl` of the selected frame (packed: the record's pitch and stride)
  long row_bytes = (long)s.Ws * XB;
  long frame_bytes = (long)s.Hs * row_bytes;
  if constexpr (PK::kPacked) row_bytes = pk.row_bytes, frame_bytes = pk.frame_bytes;
  const long first = (s.clip_frame0 + s.ts) * frame_bytes + (long)a.xs0 * XB;
  const long plane_bytes = INTER ? 0 : (long)s.N * frame_bytes;
  auto row_addr = [&](int y, int pl) -> uintptr_t { return s.src + first + (long)pl * plane_bytes + (long)y * row_bytes; };

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
        const uintptr_t ad = row_addr(a.ys0 + slot, pl);
        if (ch * 16 < (int)(ad & 15) + span_bytes) {
          val[u] = *reinterpret_cast<const u32x4*>((ad & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = sp * pitch + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- sum ---------------------------------------------------------------------------------------------------
  float sc[4], sh[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = (d.ch_scale && c < d.C) ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift && c < d.C) ? d.ch_shift[c] : 0.f;
  }
  // the low address bits of a staged row: 32-bit arithmetic keeps `addr & 15`
  const unsigned rb32 = (unsigned)row_bytes, pb32 = (unsigned)plane_bytes, a32 = (unsigned)(s.src + first);
  float* res = reinterpret_cast<float*>(lds + g.out_base);
  const int npix = a.nrows * a.ncols;
  for (int p = tid; p < npix; p += kRsThreads) {
    const int r = p / a.ncols, x = p - r * a.ncols;
    int wy0, wy1, wx0, wx1;
    rs_area_win(s.yoff + a.row0 + r, s.Hs, Hn, wy0, wy1);
    rs_area_win(s.xoff + a.col0 + x, s.Ws, Wn, wx0, wx1);
    float tot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int cx = wx0; cx < wx1; ++cx) {
      float cs[4] = {0.f, 0.f, 0.f, 0.f};          // the column sums, rows ascending
      const int ox = (cx - a.xs0) * XB;
      for (int cy = wy0; cy < wy1; ++cy) {
        const int slot = cy - a.ys0;
        if constexpr (PK::kPacked && PK::PB == 4) {   // one dword read per tap, the channels out of the register
          const int lo = (int)((a32 + (unsigned)cy * rb32) & 15u);
          const unsigned w = rs_px4(lds, slot * pitch + lo + ox);
#pragma unroll
          for (int c = 0; c < 3; ++c) cs[c] += rs_px4_ch(w, pk.o[c]);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < d.C) {
              const int pl = INTER ? 0 : c;
              const int lo = (int)((a32 + (unsigned)pl * pb32 + (unsigned)cy * rb32) & 15u);
              cs[c] += rs_tap<S>(lds, (slot * planes + pl) * pitch + lo + ox + (INTER ? rs_ch_byte(pk, c) : 0));
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) tot[c] += cs[c];  // columns ascending
    }
    const float cnt = (float)((wy1 - wy0) * (wx1 - wx0));
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < d.C) res[(c * g.R + r) * g.X + x] = fmaf(tot[c] / cnt, sc[c], sh[c]);
  }
  __syncthreads();

  ar_store<FORM, D>(res, g, a, d, d.C, zi, t);
}

// CSTEP / FORM / D / SMP / SUB / ARR: as rs_strip_yuv; the staged rows of RsMacro span the macropixels [xs0 >> 1, (xs1 - 1) >> 1].
template <int CSTEP, int FORM, typename D, typename SMP, typename SUB = RsSub420, typename ARR = RsPlanes>
__device__ __forceinline__ void ar_tile_yuv(unsigned char* lds, const ArLaunch& g, const RsYuvSrc& s, int Hn, int Wn, const RsDst& d,
                                            const float* yuv2rgb, int zi, int t, const SUB& sub = SUB()) {
  constexpr int CP = CSTEP == 1 ? 2 : 1;           // staged chroma planes
  constexpr int SB = (int)sizeof(SMP);             // bytes from one luma column to the next
  constexpr int CB = CSTEP * SB;                   // bytes from one chroma column to the next
  const int tid = threadIdx.x;
  const ArTile a = ar_tile(g, d.Ho, d.Wo, s.yoff, s.xoff, s.Hs, s.Ws, Hn, Wn);
  if (a.nrows <= 0 || a.ncols <= 0) return;
  const int pitch_y = g.pitch, pitch_c = g.pitch_c, c_base = g.c_base;
  const int cr0 = a.ys0 >> sub.csy, cc0 = a.xs0 >> sub.csx;
  const int nslots = a.ys1 - a.ys0, ncslots = ARR::kMacro ? 0 : ((a.ys1 - 1) >> sub.csy) - cr0 + 1;
  const int span_y = ARR::kMacro ? (((a.xs1 - 1) >> 1) - cc0 + 1) * CB : (a.xs1 - a.xs0) * SB;   // macropixels: one staged row, the span of both
  const int span_c = (((a.xs1 - 1) >> sub.csx) - cc0 + 1) * CB;
  if (nslots > g.rows || ncslots > g.rows_c || span_y + 15 > pitch_y || (!ARR::kMacro && span_c + 15 > pitch_c)) return;

  const uintptr_t frame = s.src + s.frame_off;
  // the first staged byte of source row y: luma column xs0, or the macropixel that holds it
  auto y_addr = [&](int y) -> uintptr_t { return frame + (long)y * s.y_pitch + (ARR::kMacro ? cc0 * CB : a.xs0 * SB); };
  auto c_addr = [&](int cy, int pl) -> uintptr_t {
    return frame + (pl == 0 ? s.c_off_a : s.c_off_b) + (long)cy * s.c_pitch + (long)cc0 * CB;
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
        const bool luma = ARR::kMacro || idx < total_y;
        const int j = luma ? idx : idx - total_y;
        const int cpr = luma ? cpr_y : cpr_c;
        const int sp = j / cpr, ch = j - sp * cpr;             // luma: sp = slot; chroma: sp = slot * CP + plane
        const int slot = luma ? sp : sp / CP, pl = luma ? 0 : sp - slot * CP;
        const uintptr_t ad = luma ? y_addr(a.ys0 + slot) : c_addr(cr0 + slot, pl);
        if (ch * 16 < (int)(ad & 15) + (luma ? span_y : span_c)) {
          val[u] = *reinterpret_cast<const u32x4*>((ad & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = (luma ? sp * pitch_y : c_base + sp * pitch_c) + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- sum ---------------------------------------------------------------------------------------------------
  float m[12], sc[3], sh[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = yuv2rgb[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sc[c] = d.ch_scale ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift) ? d.ch_shift[c] : 0.f;
  }
  // the low address bits of a staged row: 32-bit arithmetic keeps `addr & 15`
  const unsigned ya32 = (unsigned)(frame + (ARR::kMacro ? cc0 * CB : a.xs0 * SB)), yp32 = (unsigned)s.y_pitch, cp32 = (unsigned)s.c_pitch;
  const unsigned ua32 = (unsigned)(frame + s.c_off_a + (long)cc0 * CB), va32 = (unsigned)(frame + s.c_off_b + (long)cc0 * CB);
  // LDS byte offsets of the Y, U and V samples of source pixel (y, column offsets oyx / ocx)
  auto tap = [&](int y, int oyx, int ocx, int& oy, int& ou, int& ov) {
    oy = (y - a.ys0) * pitch_y + (int)((ya32 + (unsigned)y * yp32) & 15u) + oyx;
    if constexpr (ARR::kMacro) {                   // one staged row: U and V at their bytes of the macropixel (oyx holds luma's)
      ou = oy - oyx + s.u_byte + ocx, ov = oy - oyx + s.v_byte + ocx;
      return;
    }
    const int cr = y >> sub.csy, crow = c_base + (cr - cr0) * CP * pitch_c;
    ou = crow + (int)((ua32 + (unsigned)cr * cp32) & 15u) + s.u_byte + ocx;
    ov = crow + (CP - 1) * pitch_c + (int)((va32 + (unsigned)cr * cp32) & 15u) + s.v_byte + ocx;
  };
  float* res = reinterpret_cast<float*>(lds + g.out_base);
  const int npix = a.nrows * a.ncols;
  for (int p = tid; p < npix; p += kRsThreads) {
    const int r = p / a.ncols, x = p - r * a.ncols;
    int wy0, wy1, wx0, wx1;
    rs_area_win(s.yoff + a.row0 + r, s.Hs, Hn, wy0, wy1);
    rs_area_win(s.xoff + a.col0 + x, s.Ws, Wn, wx0, wx1);
    float tot[3] = {0.f, 0.f, 0.f};
    for (int cx = wx0; cx < wx1; ++cx) {
      float cs[3] = {0.f, 0.f, 0.f};               // the column sums of the converted, clamped taps, rows ascending
      const int ocx = ((cx >> sub.csx) - cc0) * CB;
      const int oyx = ARR::kMacro ? rs_macro_y_byte<SB>(s.u_byte) + (cx - 2 * cc0) * 2 * SB : (cx - a.xs0) * SB;
      for (int cy = wy0; cy < wy1; cy += 2) {      // two rows per call: yuv_tap2's packed pair
        const bool two = cy + 1 < wy1;
        int y0, u0, v0, y1, u1, v1;
        tap(cy, oyx, ocx, y0, u0, v0);
        tap(two ? cy + 1 : cy, oyx, ocx, y1, u1, v1);
        f32x2 rgb[3];
        yuv_tap2<SMP>(m, lds, y0, u0, v0, y1, u1, v1, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          cs[c] += rgb[c][0];
          if (two) cs[c] += rgb[c][1];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) tot[c] += cs[c];  // columns ascending
    }
    const float cnt = (float)((wy1 - wy0) * (wx1 - wx0));
#pragma unroll
    for (int c = 0; c < 3; ++c) res[(c * g.R + r) * g.X + x] = fmaf(tot[c] / cnt, sc[c], sh[c]);
  }
  __syncthreads();

  ar_store<FORM, D>(res, g, a, d, 3, zi, t);
}

}  // namespace
