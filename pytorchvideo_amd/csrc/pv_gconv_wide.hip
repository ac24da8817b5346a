// Grouped 3-D convolution with 64 or 128 channels per group (ResNeXt-3D 32x8d res5, 32x16d res4 / res5, CSN with
// stage_conv_b_width_per_group = 64 | 128):
//   nn.Conv3d(C, C, kernel, stride, padding, groups = C / gw, bias=False) [+ BatchNorm3d eval][+ ReLU | Swish],  gw = 64 | 128
// bf16 in, fp32 accumulation, bf16 out.  Same scope, weight layout ([C][taps][gw]) and plane ring as gconv_plane_kernel
// (pv_gconv.hip); what differs is where the filter lives.  One group's filter is gw * gw * taps * 2 bytes -- 72 KB to 864 KB --
// so it cannot stay in LDS for the life of the workgroup, and a group has 2 or 4 row tiles of 32 output channels:
//   * work split: a workgroup owns one clip x ONE group x a TH x TW tile of output voxels and walks T.  Its waves split the
//     group's OUTPUT CHANNELS first (gw / 32 row tiles of v_mfma_f32_32x32x16_bf16), then the tile's voxels (gw = 64: two
//     halves); a wave owns one row tile and NT column tiles of 32 voxels.  The tiles of one (clip, group) are congruent mod 8.
//   * filter: a wave's A fragments are rows of ITS 32 output channels only, so they never enter LDS: lane (r = l % 32,
//     h = l / 32) reads 16 bytes of row chi(r), tap t, input channels 16 s + 8 h of K step s straight from global / L2 into
//     operand registers, ONE TAP AHEAD of the MFMAs that use them (two register sets, gw / 16 fragments each; the tap after the
//     last is tap 0 of the next output plane).  K is enumerated tap-major, the tap is wave-uniform: no multiplied zeros.
//   * rows are permuted as in the dense GEMM kernels (chi(r) = 16 (r/4 % 2) + 4 (r / 8) + r % 4): the 16 accumulators of a
//     lane are 16 consecutive channels of one voxel -> two 16-byte stores.
//   * input: the halo tile of a plane (the group's gw channels) is staged into LDS once, into a ring of kt + 1 planes; plane
//     p + 1 is requested before the MFMAs of the output that plane p completes and written behind them.  Where not even the
//     smallest tile fits with kt + 1 planes (gw = 128 under a spatial stride of 2 with kt = 3) the ring has kt planes and a
//     second barrier separates the MFMAs from the write of plane p + 1; the request is still in flight under the MFMAs.
//   * B operand: one ds_read_b128 per lane and K step -- lane (n, h) reads channels 16 s + 8 h of output voxel n displaced by
//     the tap; it feeds a 32-row tile.  Voxel stride gw * 2 + 16 bytes (16 B x odd), stride-2 columns even-first / odd-second.
//   * dilation (1, dh, dw) (DIL = true): the polyphase split of gconv_plane_kernel -- the workgroup's tile is a tile of ONE
//     phase (rh, rw) of the outputs, and the phase enters only the image address of a staged voxel row and the store address.
//     The filter stream does not depend on the phase; the dh dw phases of a group are neighbours in the grid, so the rows they
//     all stream stay in one XCD's L2.
#include "pv_common.h"

bool pv_gconv_in_scope(const pv_conv3d_desc& d);   // pv_gconv.hip: everything gconv_configure demands but the group width

namespace {

constexpr int kGwStage = 12;            // 16-byte chunks of a halo plane a thread keeps in flight
constexpr unsigned kGwOob = 0x80000000u;
constexpr long kGwLdsMax = 160 * 1024;
typedef unsigned int gw_u32x4 __attribute__((ext_vector_type(4)));

struct GWide {
  const void* x; const void* w; void* y;
  const float* scale; const float* shift;
  long x_bs, y_bs;
  int ldx, ldy;
  int B, Ti, Hi, Wi, C, To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw, act;
  // launch configuration (gwide_configure)
  int TH, TW, NT, nwaves;      // output tile; TH * TW = 32 * NT * (nwaves / (gw / 32)) voxels
  int R;                       // planes of the ring: kt + 1, or kt (second barrier per plane)
  int tiles_h, tiles_w, groups, units;   // units = B * groups
  int HTH, HTW, HTWh, hcols;   // halo rows, column slots per row, slots per column parity (sw = 2), halo columns that exist
  int vs, plane_bytes, lds;    // LDS voxel stride (bytes), bytes of a ring slot, dynamic LDS
  // dilated form only (DIL): dilation in H / W, tiles of all phases of one unit
  int dh, dw, ptiles;
};

// GW: channels per group; NT: 32-voxel column tiles of a wave; DIL: the tile is a tile of one phase of the dilated conv.
template <int GW, int NT, bool DIL>
__global__ __launch_bounds__(256) void gconv_wide_kernel(const GWide d) {
  constexpr int RT = GW / 32, KS = GW / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int taps = d.kt * d.kh * d.kw, R = d.R;
  float* sc_s = reinterpret_cast<float*>(smem);
  float* sh_s = sc_s + GW;
  int* tap_s = reinterpret_cast<int*>(sh_s + GW);         // [32]: ring byte offset of a tap (dt planes + dh rows + dw columns)
  unsigned char* ring = reinterpret_cast<unsigned char*>(tap_s + 32);

  const int tid = threadIdx.x, nthr = d.nwaves * 64;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n32 = lane & 31, h = lane >> 5;
  const int rt = wave % RT, vsp = wave / RT;               // the wave's row tile, its share of the tile's voxels
  // the tiles of one (clip, group) share halos: they are consecutive slots of ONE residue mod 8 (one XCD)
  const int ntile = DIL ? d.ptiles : d.tiles_h * d.tiles_w;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int unit = (slot / ntile) * 8 + xcd, tile = slot % ntile;
  if (unit >= d.units) return;                             // the grid is padded to 8 units
  const int b = unit / d.groups, c0 = (unit % d.groups) * GW;
  PvPhaseTile pp{0, 0, d.Ho, d.Wo, (tile / d.tiles_w) * d.TH, (tile % d.tiles_w) * d.TW};
  if constexpr (DIL) pp = pv_phase_tile(tile, d.Ho, d.Wo, d.dh, d.dw, d.TH, d.TW);
  const int ho0 = pp.ho0, wo0 = pp.wo0;                    // DIL: in the coordinates of phase (pp.rh, pp.rw)

  const bf16_t* xb = static_cast<const bf16_t*>(d.x) + (long)b * d.x_bs;
  bf16_t* yb = static_cast<bf16_t*>(d.y) + (long)b * d.y_bs;
  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(xb), 0, (int)((((unsigned)d.Ti * d.Hi * d.Wi - 1u) * (unsigned)d.ldx + (unsigned)d.C) * 2u), 0x00020000);
  __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
      yb, 0, (int)((((unsigned)d.To * d.Ho * d.Wo - 1u) * (unsigned)d.ldy + (unsigned)d.C) * 2u), 0x00020000);
  __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(d.w), 0, (int)((unsigned)d.C * (unsigned)taps * (unsigned)GW * 2u), 0x00020000);

  // ---- the wave's filter rows: lane (r, h) streams row chi(r) of row tile rt, 8 input channels per K step ----
  const int chi = 16 * ((n32 >> 2) & 1) + 4 * (n32 >> 3) + (n32 & 3);
  const unsigned w_lane = (((unsigned)(c0 + rt * 32 + chi) * taps) * GW + h * 8) * 2u;
  bf16x8 w0[KS], w1[KS];
  auto load_w = [&](bf16x8 (&wf)[KS], int tap) {
    const unsigned o = w_lane + (unsigned)tap * (GW * 2u);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      wf[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(o + s * 32u), 0, 0));
  };

  // ---- per-thread constants of the plane staging: chunk j is (halo row, column slot, 8-channel chunk), the same for every plane
  unsigned soff[kGwStage];   // byte offset inside a plane of x, kGwOob: outside the image -> zero
  int sdst[kGwStage];        // byte offset inside a ring slot, -1: no chunk
  constexpr int nch = GW / 8;
  const int stage_total = d.HTH * d.HTW * nch;
#pragma unroll
  for (int j = 0; j < kGwStage; ++j) {
    const int id = tid + j * nthr;
    const int v = id / nch, ch = id - v * nch;
    const int hr = v / d.HTW, sl = v - hr * d.HTW;
    const int hc = d.sw == 2 ? (sl % d.HTWh) * 2 + sl / d.HTWh : sl;   // even columns first, odd columns second
    // DIL: halo voxel (hr, hc) of the phase is image voxel ((.) dh + rh, (.) dw + rw); the stride is 1 wherever dh / dw is not
    const int hh = DIL ? (ho0 * d.sh + hr) * d.dh + pp.rh - d.ph : ho0 * d.sh - d.ph + hr;
    const int ww = DIL ? (wo0 * d.sw + hc) * d.dw + pp.rw - d.pw : wo0 * d.sw - d.pw + hc;
    const bool ok = id < stage_total && hc < d.hcols && (unsigned)hh < (unsigned)d.Hi && (unsigned)ww < (unsigned)d.Wi;
    soff[j] = ok ? (((unsigned)hh * d.Wi + ww) * (unsigned)d.ldx + c0 + ch * 8) * 2u : kGwOob;
    sdst[j] = id < stage_total ? v * d.vs + ch * 16 : -1;
  }
  const unsigned x_plane = (unsigned)d.Hi * d.Wi * (unsigned)d.ldx * 2u;
  gw_u32x4 sv[kGwStage];
  auto request = [&](int p) {                 // plane p of x -> registers; frames outside the clip read as zeros
    const bool in = (unsigned)p < (unsigned)d.Ti;
    const unsigned po = in ? (unsigned)p * x_plane : 0u;
#pragma unroll
    for (int j = 0; j < kGwStage; ++j)
      if (j * nthr < stage_total)
        sv[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(in ? soff[j] + po : kGwOob), 0, 0);
  };
  auto commit = [&](int p) {                  // registers -> ring slot (p + pt) % R
    unsigned char* dst = ring + ((p + d.pt) % R) * d.plane_bytes;
#pragma unroll
    for (int j = 0; j < kGwStage; ++j)
      if (j * nthr < stage_total && sdst[j] >= 0) *reinterpret_cast<gw_u32x4*>(dst + sdst[j]) = sv[j];
  };
  // planes no output needs (kt < st) are neither requested nor written
  auto needed = [&](int p) { return (p + d.pt) % d.st < d.kt; };

  const int p_first = -d.pt, p_last = (d.To - 1) * d.st - d.pt + d.kt - 1;
  request(p_first);
  load_w(w0, 0);      // tap 0 of the first output plane

  // ---- BN scale / shift of the group, tap table ----
  if (tid < GW) {
    sc_s[tid] = d.scale ? d.scale[c0 + tid] : 1.f;
    sh_s[tid] = d.shift ? d.shift[c0 + tid] : 0.f;
  }
  if (tid < 32) {
    const int tap = tid < taps ? tid : 0;
    const int dt = tap / (d.kh * d.kw), r2 = tap - dt * d.kh * d.kw, dh = r2 / d.kw, dw = r2 - dh * d.kw;
    const int col = d.sw == 2 ? (dw & 1) * d.HTWh + (dw >> 1) : dw;
    tap_s[tid] = dt * d.plane_bytes + (dh * d.HTW + col) * d.vs;
  }
  pv_wait_loads();
  commit(p_first);

  // ---- the wave's NT 32-voxel tiles: LDS offset of the voxel's tap (0,0,0) + the lane's channels, output offset ----
  int vb[NT];
  unsigned yo[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int m = (vsp * NT + i) * 32 + n32;
    const int r = m / d.TW, c = m - r * d.TW;
    vb[i] = (r * d.sh * d.HTW + c) * d.vs + h * 16;
    const int ho = ho0 + r, wo = wo0 + c;
    if constexpr (DIL)
      yo[i] = (ho < pp.Hop && wo < pp.Wop)
                  ? (((unsigned)(ho * d.dh + pp.rh) * d.Wo + (wo * d.dw + pp.rw)) * (unsigned)d.ldy + c0 + rt * 32 + h * 16) * 2u : kGwOob;
    else
      yo[i] = (ho < d.Ho && wo < d.Wo) ? (((unsigned)ho * d.Wo + wo) * (unsigned)d.ldy + c0 + rt * 32 + h * 16) * 2u : kGwOob;
  }
  const unsigned y_plane = (unsigned)d.Ho * d.Wo * (unsigned)d.ldy * 2u;
  const int ring_bytes = R * d.plane_bytes;

  int to = 0;
  auto plane_out = [&]() {
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    const int base = ((to * d.st) % R) * d.plane_bytes;    // slot of plane to * st - pt
    auto mfmas = [&](const bf16x8 (&wf)[KS], int tap) {
      const int tp = base + tap_s[tap];
      int ad[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        ad[i] = tp + vb[i];
        ad[i] = ad[i] >= ring_bytes ? ad[i] - ring_bytes : ad[i];
      }
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const bf16x8 xf = *reinterpret_cast<const bf16x8*>(ring + ad[i] + s * 32);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], xf, acc[i], 0, 0, 0);
        }
    };
    // w0 holds tap 0 on entry (requested behind the last tap of the plane before); the other set is requested a tap ahead
    for (int tap = 0; tap < taps; tap += 2) {
      if (tap + 1 < taps) {
        load_w(w1, tap + 1);
        mfmas(w0, tap);
        load_w(w0, tap + 2 < taps ? tap + 2 : 0);
        mfmas(w1, tap + 1);
      } else {
        mfmas(w0, tap);
        load_w(w0, 0);
      }
    }
    // ---- epilogue: lane (n32, h) holds channels 16 h .. 16 h + 15 of row tile rt for each of its voxels ----
    const unsigned yt = (unsigned)to * y_plane;
    const int cl = rt * 32 + h * 16;
    f32x4 s4[4], h4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s4[k] = *reinterpret_cast<const f32x4*>(sc_s + cl + 4 * k);
      h4[k] = *reinterpret_cast<const f32x4*>(sh_s + cl + 4 * k);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = acc[i][j] * s4[j >> 2][j & 3] + h4[j >> 2][j & 3];
      pv_apply_act_n<true>(v, d.act);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        bf16x8 ob;
#pragma unroll
        for (int j = 0; j < 8; ++j) ob[j] = (bf16_t)v[8 * k + j];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gw_u32x4, ob), ry,
                                               (int)(yo[i] != kGwOob ? yo[i] + yt + 16u * k : kGwOob), 0, 0);
      }
    }
  };

  for (int p = p_first; p <= p_last; ++p) {
    const bool more = p + 1 <= p_last && needed(p + 1);
    if (more) request(p + 1);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // plane p is in the ring; with kt + 1 slots, slot (p + 1) % R is free: every wave is done with the output before
    if (p == to * d.st - d.pt + d.kt - 1) {
      plane_out();
      ++to;
    }
    if (R == d.kt) __syncthreads();   // kt slots: plane p + 1 replaces the oldest plane this output has just read
    if (more) commit(p + 1);
  }
}

struct GwTile { int th, tw, nt, nwaves; };

// Geometry -> launch configuration; false where the kernel does not serve the shape.
bool gwide_configure(const pv_conv3d_desc& d, GWide& g) {
  if (!pv_gconv_in_scope(d)) return false;
  const int gw = d.cout / d.groups;
  if (gw != 64 && gw != 128) return false;

  g = GWide{};
  g.x = d.x; g.w = d.w; g.y = d.y; g.scale = d.scale; g.shift = d.shift;
  g.x_bs = d.x_bs; g.y_bs = d.y_bs; g.ldx = d.ldx; g.ldy = d.ldy;
  g.B = d.B; g.Ti = d.Ti; g.Hi = d.Hi; g.Wi = d.Wi; g.C = d.cout; g.To = d.To; g.Ho = d.Ho; g.Wo = d.Wo;
  g.kt = d.kt; g.kh = d.kh; g.kw = d.kw; g.st = d.st; g.sh = d.sh; g.sw = d.sw; g.pt = d.pt; g.ph = d.ph; g.pw = d.pw;
  g.act = d.act;
  g.groups = d.groups;
  g.dh = d.dil_h > 1 ? d.dil_h : 1; g.dw = d.dil_w > 1 ? d.dil_w : 1;
  const int Wop = pv_phase_extent(d.Wo, g.dw, 0);    // columns of the widest phase (Wo itself where undilated)
  // Tiles, largest first (a larger tile streams the filter less often per output voxel); planes of at most 8 columns take the
  // 8-column tiles only.  The first tile whose ring of kt + 1 halo planes and staging registers fit is taken; if none does,
  // the first that fits with kt planes.
  static const GwTile kTiles64[4] = {{8, 16, 2, 4}, {4, 16, 1, 4}, {8, 8, 1, 4}, {4, 8, 1, 2}};
  static const GwTile kTiles128[4] = {{8, 16, 4, 4}, {4, 16, 2, 4}, {8, 8, 2, 4}, {4, 8, 1, 4}};
  const GwTile* tiles = gw == 64 ? kTiles64 : kTiles128;
  for (int R = d.kt + 1; R >= d.kt; --R) {
    for (int t = Wop <= 8 ? 2 : 0; t < 4; ++t) {
      g.TH = tiles[t].th; g.TW = tiles[t].tw; g.NT = tiles[t].nt; g.nwaves = tiles[t].nwaves; g.R = R;
      g.hcols = (g.TW - 1) * d.sw + d.kw;
      g.HTH = (g.TH - 1) * d.sh + d.kh;
      g.HTWh = (g.hcols + 1) / 2;
      g.HTW = d.sw == 2 ? 2 * g.HTWh : g.hcols;
      g.vs = gw * 2 + 16;
      g.plane_bytes = g.HTH * g.HTW * g.vs;
      const long lds = gw * 8 + 128 + (long)R * g.plane_bytes;
      if (lds > kGwLdsMax) continue;
      if ((long)g.HTH * g.HTW * (gw / 8) > (long)kGwStage * g.nwaves * 64) continue;
      g.lds = (int)lds;
      g.tiles_h = (d.Ho + g.TH - 1) / g.TH; g.tiles_w = (d.Wo + g.TW - 1) / g.TW;
      const long units = (long)d.B * d.groups;
      g.ptiles = pv_phase_tiles(d.Ho, g.dh, g.TH) * pv_phase_tiles(d.Wo, g.dw, g.TW);   // = tiles_h * tiles_w where undilated
      if ((units + 7) / 8 * 8 * g.ptiles > 0x7fffffffL) return false;
      g.units = (int)units;
      return true;
    }
  }
  return false;
}

template <int GW, int NT, bool DIL> int gwide_launch_as(const GWide& g, hipStream_t s) {
  const unsigned grid = (unsigned)((g.units + 7) / 8 * 8 * g.ptiles);
  if (g.lds > 64 * 1024)
    PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gconv_wide_kernel<GW, NT, DIL>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, g.lds));
  PV_LAUNCH((gconv_wide_kernel<GW, NT, DIL>), dim3(grid), dim3(g.nwaves * 64), (size_t)g.lds, s, g);
  return pv_launch_status();
}

template <int GW, int NT> int gwide_launch(const GWide& g, hipStream_t s) {
  return g.dh * g.dw > 1 ? gwide_launch_as<GW, NT, true>(g, s) : gwide_launch_as<GW, NT, false>(g, s);
}

}  // namespace

int pv_gconv_wide_supported(const pv_conv3d_desc& d) {
  GWide g;
  return gwide_configure(d, g) ? 1 : 0;
}

int pv_gconv_wide_try(const pv_conv3d_desc& d, hipStream_t s) {
  GWide g;
  if (!gwide_configure(d, g)) return PV_ERR_UNSUPPORTED;
  if (d.cout / d.groups == 64) return g.NT == 2 ? gwide_launch<64, 2>(g, s) : gwide_launch<64, 1>(g, s);
  return g.NT == 4 ? gwide_launch<128, 4>(g, s) : g.NT == 2 ? gwide_launch<128, 2>(g, s) : gwide_launch<128, 1>(g, s);
}
