// Grouped 3-D convolution with 16 or 32 channels per group (ResNeXt-3D conv_b, the wide-group CSN variants):
//   nn.Conv3d(C, C, kernel, stride, padding, groups = C / gw, bias=False) [+ BatchNorm3d eval][+ ReLU | Swish],  gw = 16 | 32
// (create_resnet / create_slowfast(stage_conv_b_num_groups=...), models/resnet.py:98-132; create_csn(
// stage_conv_b_width_per_group=...), models/csn.py:34,169).  bf16 in, fp32 accumulation, bf16 out.  (gw = 64 | 128: the kernel
// of pv_gconv_wide.hip, reached through the two entry points at the end of this file.)
//
// Per group the conv is an implicit GEMM with N = gw output channels and K = taps * gw: with gw = 16 one
// v_mfma_f32_16x16x32_bf16 covers two taps of a group, with gw = 32 one tap.  27 * gw / (stride^2 + 1) FLOP/B sits around
// the ridge, so every input plane is read from HBM ONCE and the taps are gathered from LDS:
//   * work split: a workgroup owns one clip x a channel SLAB of whole groups (<= 64 channels at gw = 16, 32 at gw = 32; the
//     last slab may be ragged) x a TH x TW tile of output voxels, and walks T.  Groups never interact, so the slab is simply
//     a grid dimension; the tiles of one (clip, slab) -- the workgroups whose halos overlap -- are congruent mod 8: one XCD's
//     L2 serves the overlap.
//   * input: the halo tile of a plane (slab channels only) is staged into LDS once, into a ring of kt + 1 planes; plane p + 1
//     is requested (buffer loads, rows / columns / frames outside the image zero-filled by the range check: no bounds
//     branches) before the MFMAs of the output that plane p completes, and written behind them.  One barrier per plane.
//   * B operand of a K step: one ds_read_b128 per lane -- lane (n = l % 16, q = l / 16) reads 8 consecutive channels of output
//     voxel n displaced by the step's tap (gw = 16: taps 2s, 2s + 1 for q < 2, q >= 2; gw = 32: tap s, channels 8q).  The voxel
//     stride in LDS is slab bytes + 16 (16 B x odd): the 16 lanes of a read hit 16 different 16-byte bank groups; under
//     W stride 2 the columns are stored even-first / odd-second, so a tile row is still consecutive voxels.
//   * filter: the slab's weights ([C][taps][gw] in memory) sit in LDS in A-FRAGMENT order for the life of the workgroup:
//     fragment (row tile, K step) is 64 x 16 B, lane l reads chunk l -- conflict-free by construction.  An odd tap count at
//     gw = 16 gets one zero tap (zero-filled by the range check when the slab is staged), not a branch.
//   * epilogue: fp32 scale / shift / activation, one rounding, 16-byte stores.  gw = 32: the two row tiles of the group are
//     interleaved in groups of 4 rows (as in pv_lateral.hip), so a lane's accumulators are 8 consecutive channels.  gw = 16: a
//     row tile is one group, so lanes q and q ^ 1 trade halves of their two voxel tiles instead (4 cross-lane moves).
//   * dilation (1, dh, dw), dh, dw <= 4, at stride 1 where dilated (the res5 conv_b of a detection backbone: DIL = true): a
//     polyphase split, not a wider halo.  The outputs with h = i dh + rh, w = j dw + rw are an undilated conv of the inputs of one
//     residue, so a workgroup owns (clip, slab, PHASE (rh, rw), tile of that phase's outputs) and only the two places that form
//     a global address know: halo row hr of the tile is image row (ho0 + hr) dh + rh - ph, output (i, j) is stored at
//     ((ho0 + i) dh + rh, (wo0 + j) dw + rw).  Ring, voxel stride, tap table, operand reads and the K loop are the undilated
//     kernel's; the halo stays (TH - 1) + kh rows.  Phases are tiled on their own extents (pv_phase_tile, pv_common.h); all
//     tiles of all phases of a (clip, slab) sit on one XCD residue, phase-major.
#include "pv_common.h"

namespace {

constexpr int kGcStage = 10;            // 16-byte chunks of a halo plane a thread keeps in flight
constexpr int kGcFilterBatch = 7;       // ... and of the filter slab per start-up batch
constexpr unsigned kGcOob = 0x80000000u;
constexpr long kGcLdsMax = 160 * 1024;
typedef unsigned int gc_u32x4 __attribute__((ext_vector_type(4)));
template <int N> struct GcInt { static constexpr int value = N; };

struct GConv {
  const void* x; const void* w; void* y;
  const float* scale; const float* shift;
  long x_bs, y_bs;
  int ldx, ldy;
  int B, Ti, Hi, Wi, C, To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw, act;
  // launch configuration (gconv_configure)
  int TH, TW, nwaves;          // output tile, TH * TW = 32 * nwaves voxels
  int CS;                      // channels of a full slab
  int tiles_h, tiles_w, nslabs, units;   // units = B * nslabs
  int HTH, HTW, HTWh;          // halo rows, column SLOTS per row, slots per column parity (sw = 2)
  int hcols;                   // halo columns that exist: (TW - 1) * sw + kw
  int vs, plane_bytes, ksteps; // LDS voxel stride (bytes), bytes of a ring slot, K steps
  int lds;
  // dilated form only (DIL): dilation in H / W, tiles of all phases of one unit
  int dh, dw, ptiles;
};

// GW: channels per group.  NG x TPG 16-row MFMA tiles per slab: 4 groups x 1 tile, or 1 group x 2 tiles.  DIL: the workgroup's
// tile is a tile of one phase of the dilated conv.
template <int GW, bool DIL>
__global__ __launch_bounds__(256) void gconv_plane_kernel(const GConv d) {
  constexpr int NG = GW == 16 ? 4 : 1, TPG = GW / 16, MT = NG * TPG, NTW = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int taps = d.kt * d.kh * d.kw, R = d.kt + 1;
  const int mts = d.CS / 16;                               // row tiles of a full slab
  unsigned char* w_s = smem;                               // [mts][ksteps] fragments of 1 KB
  float* sc_s = reinterpret_cast<float*>(smem + mts * d.ksteps * 1024);
  float* sh_s = sc_s + d.CS;
  int* tap_s = reinterpret_cast<int*>(sh_s + d.CS);       // [32]: ring byte offset of a tap (dt planes + dh rows + dw columns)
  unsigned char* ring = reinterpret_cast<unsigned char*>(tap_s + 32);

  const int tid = threadIdx.x, nthr = d.nwaves * 64;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, q = lane >> 4;
  // the tiles of one (clip, slab) share halos: they are consecutive slots of ONE residue mod 8 (one XCD)
  const int ntile = DIL ? d.ptiles : d.tiles_h * d.tiles_w;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int unit = (slot / ntile) * 8 + xcd, tile = slot % ntile;
  if (unit >= d.units) return;                             // the grid is padded to 8 units
  const int b = unit / d.nslabs, c0 = (unit % d.nslabs) * d.CS;
  PvPhaseTile pp{0, 0, d.Ho, d.Wo, (tile / d.tiles_w) * d.TH, (tile % d.tiles_w) * d.TW};
  if constexpr (DIL) pp = pv_phase_tile(tile, d.Ho, d.Wo, d.dh, d.dw, d.TH, d.TW);
  const int ho0 = pp.ho0, wo0 = pp.wo0;                    // DIL: in the coordinates of phase (pp.rh, pp.rw)
  const int live = (min(d.CS, d.C - c0)) / GW;             // groups of this slab that exist

  const bf16_t* xb = static_cast<const bf16_t*>(d.x) + (long)b * d.x_bs;
  bf16_t* yb = static_cast<bf16_t*>(d.y) + (long)b * d.y_bs;
  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(xb), 0, (int)((((unsigned)d.Ti * d.Hi * d.Wi - 1u) * (unsigned)d.ldx + (unsigned)d.C) * 2u), 0x00020000);
  __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
      yb, 0, (int)((((unsigned)d.To * d.Ho * d.Wo - 1u) * (unsigned)d.ldy + (unsigned)d.C) * 2u), 0x00020000);
  __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(d.w), 0, (int)((unsigned)d.C * (unsigned)taps * (unsigned)GW * 2u), 0x00020000);

  // ---- per-thread constants of the plane staging: chunk j is (halo row, column slot, 8-channel chunk), the same for every plane
  unsigned soff[kGcStage];   // byte offset inside a plane of x, kGcOob: outside the image / the slab -> zero
  int sdst[kGcStage];        // byte offset inside a ring slot, -1: no chunk
  const int nch = d.CS / 8, stage_total = d.HTH * d.HTW * nch;
#pragma unroll
  for (int j = 0; j < kGcStage; ++j) {
    const int id = tid + j * nthr;
    const int v = id / nch, ch = id - v * nch;
    const int hr = v / d.HTW, sl = v - hr * d.HTW;
    const int hc = d.sw == 2 ? (sl % d.HTWh) * 2 + sl / d.HTWh : sl;   // even columns first, odd columns second
    // DIL: halo voxel (hr, hc) of the phase is image voxel ((.) dh + rh, (.) dw + rw); the stride is 1 wherever dh / dw is not
    const int h = DIL ? (ho0 * d.sh + hr) * d.dh + pp.rh - d.ph : ho0 * d.sh - d.ph + hr;
    const int w = DIL ? (wo0 * d.sw + hc) * d.dw + pp.rw - d.pw : wo0 * d.sw - d.pw + hc;
    const bool ok = id < stage_total && hc < d.hcols && (unsigned)h < (unsigned)d.Hi && (unsigned)w < (unsigned)d.Wi && c0 + ch * 8 < d.C;
    soff[j] = ok ? (((unsigned)h * d.Wi + w) * (unsigned)d.ldx + c0 + ch * 8) * 2u : kGcOob;
    sdst[j] = id < stage_total ? v * d.vs + ch * 16 : -1;
  }
  const unsigned x_plane = (unsigned)d.Hi * d.Wi * (unsigned)d.ldx * 2u;
  gc_u32x4 sv[kGcStage];
  auto request = [&](int p) {                 // plane p of x -> registers; frames outside the clip read as zeros
    const bool in = (unsigned)p < (unsigned)d.Ti;
    const unsigned po = in ? (unsigned)p * x_plane : 0u;
#pragma unroll
    for (int j = 0; j < kGcStage; ++j)
      if (j * nthr < stage_total)
        sv[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(in ? soff[j] + po : kGcOob), 0, 0);
  };
  auto commit = [&](int p) {                  // registers -> ring slot (p + pt) % R
    unsigned char* dst = ring + ((p + d.pt) % R) * d.plane_bytes;
#pragma unroll
    for (int j = 0; j < kGcStage; ++j)
      if (j * nthr < stage_total && sdst[j] >= 0) *reinterpret_cast<gc_u32x4*>(dst + sdst[j]) = sv[j];
  };
  // planes no output needs (kt < st) are neither requested nor written
  auto needed = [&](int p) { return (p + d.pt) % d.st < d.kt; };

  const int p_first = -d.pt, p_last = (d.To - 1) * d.st - d.pt + d.kt - 1;
  request(p_first);   // in flight under the filter staging

  // ---- filter slab -> A fragments, BN scale / shift, tap table ----
  {
    const int total = mts * d.ksteps * 64;
    for (int i0 = tid; i0 < total; i0 += nthr * kGcFilterBatch) {
      gc_u32x4 fv[kGcFilterBatch];
#pragma unroll
      for (int j = 0; j < kGcFilterBatch; ++j) {
        const int id = i0 + j * nthr;
        const int l = id & 63, f = id >> 6, mt = f / d.ksteps, s = f - mt * d.ksteps;
        const int m = l & 15, fq = l >> 4;
        int c, tap, ci;
        if constexpr (GW == 16) {
          c = c0 + mt * 16 + m; tap = 2 * s + (fq >> 1); ci = (fq & 1) * 8;
        } else {   // rows of the group's two tiles interleaved in groups of 4: a lane's accumulators are 8 consecutive channels
          c = c0 + (mt >> 1) * 32 + (m >> 2) * 8 + (mt & 1) * 4 + (m & 3); tap = s; ci = fq * 8;
        }
        const bool ok = id < total && c < d.C && tap < taps;
        fv[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(ok ? (((unsigned)c * taps + tap) * GW + ci) * 2u : kGcOob), 0, 0);
      }
#pragma unroll
      for (int j = 0; j < kGcFilterBatch; ++j) {
        const int id = i0 + j * nthr;
        if (id < total) *reinterpret_cast<gc_u32x4*>(w_s + (size_t)id * 16) = fv[j];
      }
    }
    if (tid < d.CS) {
      const int c = c0 + tid;
      const int cc = c < d.C ? c : 0;
      const float sc = d.scale ? d.scale[cc] : 1.f, sh = d.shift ? d.shift[cc] : 0.f;
      sc_s[tid] = c < d.C ? sc : 0.f;
      sh_s[tid] = c < d.C ? sh : 0.f;
    }
    if (tid < 32) {
      // the zero tap of an odd count reads where tap 0 reads (its weights are zeros): an Inf or NaN input voxel under tap 0
      // gives 0 * Inf = NaN where nn.Conv3d gives Inf -- as the block-diagonal route's zero weights do
      const int tap = tid < taps ? tid : 0;
      const int dt = tap / (d.kh * d.kw), r2 = tap - dt * d.kh * d.kw, dh = r2 / d.kw, dw = r2 - dh * d.kw;
      const int col = d.sw == 2 ? (dw & 1) * d.HTWh + (dw >> 1) : dw;
      tap_s[tid] = dt * d.plane_bytes + (dh * d.HTW + col) * d.vs;
    }
  }
  // Everything requested so far has to be there now.  Said explicitly: a filter chunk past the slab's end is requested (as zeros)
  // and never stored, and a load the compiler never saw consumed stays pending in its bookkeeping -- it then waits for ALL loads
  // (the plane in flight included) at the first write of that register inside the K loop.
  pv_wait_loads();
  commit(p_first);

  // ---- the wave's two 16-voxel tiles: LDS offset of the voxel's tap (0,0,0) + the lane's channels, output offset ----
  int vb[NTW];
  unsigned yo[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int m = (wave * NTW + i) * 16 + n16;
    const int r = m / d.TW, c = m - r * d.TW;
    vb[i] = (r * d.sh * d.HTW + c) * d.vs + (GW == 16 ? (q & 1) * 16 : q * 16);
    const int ho = ho0 + r, wo = wo0 + c;
    if constexpr (DIL)
      yo[i] = (ho < pp.Hop && wo < pp.Wop)
                  ? (((unsigned)(ho * d.dh + pp.rh) * d.Wo + (wo * d.dw + pp.rw)) * (unsigned)d.ldy + c0) * 2u : kGcOob;
    else
      yo[i] = (ho < d.Ho && wo < d.Wo) ? (((unsigned)ho * d.Wo + wo) * (unsigned)d.ldy + c0) * 2u : kGcOob;
  }
  const unsigned y_plane = (unsigned)d.Ho * d.Wo * (unsigned)d.ldy * 2u;
  const int ring_bytes = R * d.plane_bytes;

  // The MFMAs and the epilogue of output plane `to`, compiled once per number of LIVE groups of the slab (1 .. NG): the K loop
  // has no branch on it, so the accumulators stay where they are and nothing in the loop waits for the plane in flight.
  int to = 0;
  auto plane_out = [&](auto lg) {
    constexpr int LG = decltype(lg)::value;
    f32x4 acc[LG * TPG][NTW];
#pragma unroll
    for (int a = 0; a < LG * TPG; ++a)
#pragma unroll
      for (int i = 0; i < NTW; ++i) acc[a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int base = ((to * d.st) % R) * d.plane_bytes;    // slot of plane to * st - pt
    for (int s = 0; s < d.ksteps; ++s) {
      const int tp = base + tap_s[GW == 16 ? 2 * s + (q >> 1) : s];
      int ad[NTW];
#pragma unroll
      for (int i = 0; i < NTW; ++i) {
        ad[i] = tp + vb[i];
        ad[i] = ad[i] >= ring_bytes ? ad[i] - ring_bytes : ad[i];
      }
#pragma unroll
      for (int g = 0; g < LG; ++g) {
        bf16x8 xf[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(ring + ad[i] + g * GW * 2);
#pragma unroll
        for (int t = 0; t < TPG; ++t) {
          const int a = g * TPG + t;
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w_s + ((a * d.ksteps + s) * 64 + lane) * 16);
#pragma unroll
          for (int i = 0; i < NTW; ++i) acc[a][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[i], acc[a][i], 0, 0, 0);
        }
      }
    }
    // ---- epilogue ----
    const unsigned yt = (unsigned)to * y_plane;
#pragma unroll
    for (int g = 0; g < LG; ++g) {
      if constexpr (GW == 32) {   // lane (n16, q): channels 8q .. 8q + 7 of both voxel tiles
        const int cl = g * 32 + q * 8;
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc_s + cl), s1 = *reinterpret_cast<const f32x4*>(sc_s + cl + 4);
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(sh_s + cl), h1 = *reinterpret_cast<const f32x4*>(sh_s + cl + 4);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = acc[2 * g][i][j] * s0[j] + h0[j];
            v[4 + j] = acc[2 * g + 1][i][j] * s1[j] + h1[j];
          }
          pv_apply_act_n<true>(v, d.act);
          bf16x8 ob;
#pragma unroll
          for (int j = 0; j < 8; ++j) ob[j] = (bf16_t)v[j];
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gc_u32x4, ob), ry,
                                                 (int)(yo[i] != kGcOob ? yo[i] + yt + (unsigned)cl * 2u : kGcOob), 0, 0);
        }
      } else {
        // lane (n16, q) holds channels 4q .. 4q + 3 of voxel n16 in both tiles.  Lanes q and q ^ 1 trade: the even one
        // ends up with channels 4q .. 4q + 7 of tile 0, the odd one with channels 4(q - 1) .. 4q + 3 of tile 1.
        const bool odd = q & 1;
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float mine = odd ? acc[g][1][j] : acc[g][0][j];
          const float got = __shfl_xor(odd ? acc[g][0][j] : acc[g][1][j], 16, 64);
          v[j] = odd ? got : mine;
          v[4 + j] = odd ? mine : got;
        }
        const int cl = g * 16 + (q >> 1) * 8;
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc_s + cl), s1 = *reinterpret_cast<const f32x4*>(sc_s + cl + 4);
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(sh_s + cl), h1 = *reinterpret_cast<const f32x4*>(sh_s + cl + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = v[j] * s0[j] + h0[j];
          v[4 + j] = v[4 + j] * s1[j] + h1[j];
        }
        pv_apply_act_n<true>(v, d.act);
        bf16x8 ob;
#pragma unroll
        for (int j = 0; j < 8; ++j) ob[j] = (bf16_t)v[j];
        const unsigned yv = odd ? yo[1] : yo[0];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gc_u32x4, ob), ry,
                                               (int)(yv != kGcOob ? yv + yt + (unsigned)cl * 2u : kGcOob), 0, 0);
      }
    }
  };

  for (int p = p_first; p <= p_last; ++p) {
    const bool more = p + 1 <= p_last && needed(p + 1);
    if (more) request(p + 1);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // plane p is in the ring; every wave is done with the output before, so slot (p + 1) % R is free
    if (p == to * d.st - d.pt + d.kt - 1) {
      if constexpr (GW == 32) plane_out(GcInt<1>());
      else if (live == 1) plane_out(GcInt<1>());
      else if (live == 2) plane_out(GcInt<2>());
      else if (live == 3) plane_out(GcInt<3>());
      else plane_out(GcInt<4>());
      ++to;
    }
    if (more) commit(p + 1);
  }
}

}  // namespace

// The scope of the grouped kernels, whatever the group width (which each kernel checks for itself: 16 / 32 here, 64 / 128 in
// pv_gconv_wide.hip).
bool pv_gconv_in_scope(const pv_conv3d_desc& d) {
  if (d.dtype != PV_BF16 || d.groups <= 1 || d.cout <= 0 || d.cout % d.groups) return false;
  const int gw = d.cout / d.groups;
  if (d.cin != d.cout) return false;
  if (d.residual || d.a_gate || d.a_act != PV_ACT_NONE || d.y_f32 || d.dwt_w || d.x2 || d.x2_cin || d.pw2_w || d.pw2_cout ||
      d.pos_spatial || d.pos_temporal || d.x_src_slot || d.c4_wpair)
    return false;
  // dilation in H / W up to 4 as a polyphase split (DIL): stride 1 in a dilated dimension, none in T
  const int dh = d.dil_h > 1 ? d.dil_h : 1, dw = d.dil_w > 1 ? d.dil_w : 1;
  if (d.dil_t > 1 || d.dil_t < 0 || d.dil_h < 0 || d.dil_w < 0 || dh > 4 || dw > 4) return false;
  const int eh = (d.kh - 1) * dh + 1, ew = (d.kw - 1) * dw + 1;   // kernel extents
  if (d.act != PV_ACT_NONE && d.act != PV_ACT_RELU && d.act != PV_ACT_SWISH) return false;
  if (d.B <= 0 || d.Ti <= 0 || d.Hi <= 0 || d.Wi <= 0 || d.To <= 0 || d.Ho <= 0 || d.Wo <= 0) return false;
  if (d.kt < 1 || d.kh < 1 || d.kw < 1 || d.kt > 27 || d.kh > 27 || d.kw > 27 || d.kt * d.kh * d.kw > 27) return false;
  if (d.st < 1 || d.st > 2 || d.sh < 1 || d.sh > 2 || d.sw < 1 || d.sw > 2) return false;
  if ((dh > 1 && d.sh != 1) || (dw > 1 && d.sw != 1)) return false;
  if (d.pt < 0 || d.ph < 0 || d.pw < 0 || d.pt > d.kt || d.ph > eh || d.pw > ew) return false;
  if ((d.Ti + 2 * d.pt - d.kt) / d.st + 1 != d.To || (d.Hi + 2 * d.ph - eh) / d.sh + 1 != d.Ho ||
      (d.Wi + 2 * d.pw - ew) / d.sw + 1 != d.Wo || d.Ti + 2 * d.pt < d.kt || d.Hi + 2 * d.ph < eh || d.Wi + 2 * d.pw < ew)
    return false;
  if (d.ldx < d.cout || d.ldy < d.cout || d.ldx % 8 || d.ldy % 8 || d.x_bs % 8 || d.y_bs % 8) return false;
  // 32-bit byte offsets inside a clip, and a grid that fits
  const long x_clip = ((long)d.Ti * d.Hi * d.Wi * d.ldx) * 2, y_clip = ((long)d.To * d.Ho * d.Wo * d.ldy) * 2;
  const int taps = d.kt * d.kh * d.kw;
  if (x_clip >= 0x7fffffffL || y_clip >= 0x7fffffffL || (long)d.cout * taps * gw * 2 >= 0x7fffffffL) return false;
  return true;
}

int pv_gconv_wide_supported(const pv_conv3d_desc& d);                 // pv_gconv_wide.hip
int pv_gconv_wide_try(const pv_conv3d_desc& d, hipStream_t s);        // pv_gconv_wide.hip

namespace {

// Geometry -> launch configuration; false where the kernel does not serve the shape.
bool gconv_configure(const pv_conv3d_desc& d, GConv& g) {
  if (!pv_gconv_in_scope(d)) return false;
  const int gw = d.cout / d.groups, taps = d.kt * d.kh * d.kw;
  if (gw != 16 && gw != 32) return false;

  g = GConv{};
  g.x = d.x; g.w = d.w; g.y = d.y; g.scale = d.scale; g.shift = d.shift;
  g.x_bs = d.x_bs; g.y_bs = d.y_bs; g.ldx = d.ldx; g.ldy = d.ldy;
  g.B = d.B; g.Ti = d.Ti; g.Hi = d.Hi; g.Wi = d.Wi; g.C = d.cout; g.To = d.To; g.Ho = d.Ho; g.Wo = d.Wo;
  g.kt = d.kt; g.kh = d.kh; g.kw = d.kw; g.st = d.st; g.sh = d.sh; g.sw = d.sw; g.pt = d.pt; g.ph = d.ph; g.pw = d.pw;
  g.act = d.act;
  g.ksteps = gw == 16 ? (taps + 1) / 2 : taps;
  g.dh = d.dil_h > 1 ? d.dil_h : 1; g.dw = d.dil_w > 1 ? d.dil_w : 1;
  const int Wop = pv_phase_extent(d.Wo, g.dw, 0);    // columns of the widest phase (Wo itself where undilated)
  // Tiles, widest first; planes of at most 8 columns take the square tile.  The first one whose filter slab, kt + 1 halo
  // planes and staging registers fit is taken; at gw = 16 a 32-channel slab is the fallback of a 64-channel one.
  static const int kTiles[3][3] = {{8, 16, 4}, {4, 16, 2}, {8, 8, 2}};
  const int cs_max = gw == 16 ? (d.cout < 64 ? d.cout : 64) : 32;
  const int slabs[2] = {cs_max, 32};
  for (int k = 0; k < (cs_max > 32 ? 2 : 1); ++k) {
    const int cs = slabs[k];
    for (int t = 0; t < 3; ++t) {
      const int* tl = kTiles[Wop <= 8 ? (t + 2) % 3 : t];
      g.TH = tl[0]; g.TW = tl[1]; g.nwaves = tl[2]; g.CS = cs;
      g.hcols = (g.TW - 1) * d.sw + d.kw;
      g.HTH = (g.TH - 1) * d.sh + d.kh;
      g.HTWh = (g.hcols + 1) / 2;
      g.HTW = d.sw == 2 ? 2 * g.HTWh : g.hcols;
      g.vs = cs * 2 + 16;
      g.plane_bytes = g.HTH * g.HTW * g.vs;
      const long lds = (long)(cs / 16) * g.ksteps * 1024 + cs * 8 + 128 + (long)(d.kt + 1) * g.plane_bytes;
      if (lds > kGcLdsMax) continue;
      if ((long)g.HTH * g.HTW * (cs / 8) > (long)kGcStage * g.nwaves * 64) continue;
      g.lds = (int)lds;
      g.tiles_h = (d.Ho + g.TH - 1) / g.TH; g.tiles_w = (d.Wo + g.TW - 1) / g.TW;
      g.nslabs = (d.cout + cs - 1) / cs;
      const long units = (long)d.B * g.nslabs;
      g.ptiles = pv_phase_tiles(d.Ho, g.dh, g.TH) * pv_phase_tiles(d.Wo, g.dw, g.TW);   // = tiles_h * tiles_w where undilated
      if ((units + 7) / 8 * 8 * g.ptiles > 0x7fffffffL) return false;
      g.units = (int)units;
      return true;
    }
  }
  return false;
}

template <int GW, bool DIL> int gconv_launch(const GConv& g, hipStream_t s) {
  const unsigned grid = (unsigned)((g.units + 7) / 8 * 8 * g.ptiles);
  if (g.lds > 64 * 1024)
    PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gconv_plane_kernel<GW, DIL>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, g.lds));
  PV_LAUNCH((gconv_plane_kernel<GW, DIL>), dim3(grid), dim3(g.nwaves * 64), (size_t)g.lds, s, g);
  return pv_launch_status();
}

}  // namespace

// 64 / 128 channels per group are the other kernel's (gconv_wide_kernel); the two ranges do not overlap
static bool gconv_is_wide(const pv_conv3d_desc& d) { return d.groups > 1 && d.cout > 0 && d.cout % d.groups == 0 && d.cout / d.groups >= 64; }

int pv_gconv_supported(const pv_conv3d_desc& d) {
  if (gconv_is_wide(d)) return pv_gconv_wide_supported(d);
  GConv g;
  return gconv_configure(d, g) ? 1 : 0;
}

int pv_gconv_try(const pv_conv3d_desc& d, hipStream_t s) {
  if (gconv_is_wide(d)) return pv_gconv_wide_try(d, s);
  GConv g;
  if (!gconv_configure(d, g)) return PV_ERR_UNSUPPORTED;
  return d.cout / d.groups == 16 ? (g.dh * g.dw > 1 ? gconv_launch<16, true>(g, s) : gconv_launch<16, false>(g, s))
                                 : (g.dh * g.dw > 1 ? gconv_launch<32, true>(g, s) : gconv_launch<32, false>(g, s));
}
