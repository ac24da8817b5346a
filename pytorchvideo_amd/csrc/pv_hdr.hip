// pv_hdr_views: the 16-bit YUV 4:2:0 ingest of pv_batch_views / pv_frame_views with every tap taken from PQ (SMPTE ST 2084) or
// HLG (BT.2100) BT.2020 R'G'B' to a BT.709-coded SDR signal before the blend (include/pv_mi355x.h, "HDR sources").  The map
// is elementwise and non-linear, so it cannot move behind the blend (a 2x downscale of black / peak-white columns would come
// out tens of codes off), and in front of the ingest it is a pass over every pixel of every frame plus an RGB copy of the
// video; on the taps it costs arithmetic only: a thread has its four converted taps in registers anyway.
//
// The kernels are the staged strip and the staged tile of pv_rs.h (rs_strip_yuv, rs_tile_yuv) with the tap map HdrMap as their
// trailing template argument: staging, coordinates, the clamp, the pinned blend, the affine map and the stores are the bodies'
// own, so everything but the map is what pv_yuv16_views computes.  One item loader serves both source forms: `frames` is
// workgroup-uniform, so the frame is `src` plus the table entry times the frame stride (whole videos) or the entry of the
// record's slice of the pointer table (frame lists), as in pv_orient.hip.  The transfer is
// a template argument -- each kernel carries one curve, which keeps the G = 8 planar forms (32 mapped taps per thread,
// unrolled) inside the instruction cache's reach: 2 transfers x 2 chroma arrangements x 5 destination forms x (strip, tile)
// = 40 kernels.
//
// The map's state -- tone[16], the caller's composition (transforms.tone_params) -- is workgroup-uniform: it is loaded through
// the kernel argument once per thread, like the matrix, and lives in scalar registers.
#include "pv_frames.h"

namespace {

// x^y for x >= 0, y > 0 on the hardware transcendentals, kept to this one form: log2(0) = -inf, y * -inf = -inf,
// exp2(-inf) = 0, so a zero base ends in 0 and never in NaN.
__device__ __forceinline__ float hdr_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }

// The tap map of include/pv_mi355x.h, steps 1 to 4, on the pair of taps yuv_tap2 hands over.  Every product and sum is
// written out (fmaf where one rounding is meant, contraction off elsewhere) so that every instantiation gives the same bits.
template <int TRANSFER> struct HdrMap {
  static constexpr bool kNone = false;
  float t[15];
  __device__ __forceinline__ explicit HdrMap(const float* __restrict__ tone) {
#pragma unroll
    for (int i = 0; i < 15; ++i) t[i] = tone[i];
  }

  __device__ __forceinline__ void one(float& r, float& g, float& b) const {
#pragma clang fp contract(off)
    float l[3] = {r * (1.f / 255.f), g * (1.f / 255.f), b * (1.f / 255.f)};
    if constexpr (TRANSFER == PV_TRANSFER_PQ) {
      constexpr float im1 = 16384.f / 2610.f, im2 = 4096.f / (2523.f * 128.f);
      constexpr float c1 = 3424.f / 4096.f, c2 = 2413.f / 4096.f * 32.f, c3 = 2392.f / 4096.f * 32.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = hdr_pow(l[c], im2);
        const float q = fmaxf(p - c1, 0.f) * __builtin_amdgcn_rcpf(fmaf(-c3, p, c2));   // c2 - c3 p >= 0.16
        l[c] = hdr_pow(q, im1) * t[0];
      }
    } else {
      constexpr float a = 0.17883277f, b4 = 1.f - 4.f * a, cc = 0.55991073f;   // c = 0.5 - a ln(4a)
      constexpr float k = 1.4426950408889634f / a;                              // exp(x / a) = exp2(x log2(e) / a)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float e = l[c];
        l[c] = e <= 0.5f ? e * e * (1.f / 3.f) : (__builtin_amdgcn_exp2f((e - cc) * k) + b4) * (1.f / 12.f);
      }
      const float ys = fmaf(0.0593f, l[2], fmaf(0.6780f, l[1], 0.2627f * l[0]));
      const float f = ys > 0.f ? hdr_pow(ys, t[1]) * t[0] : 0.f;   // Ys = 0: every s_c is 0, and 0 is the answer
#pragma unroll
      for (int c = 0; c < 3; ++c) l[c] *= f;
    }
    // the tone curve on max-RGB: the identity up to the knee t[2]
    const float m = fmaxf(fmaxf(l[0], l[1]), l[2]);
    if (m > t[2]) {
      const float kk = t[3] * (m + t[4]) * __builtin_amdgcn_rcpf((m + t[5]) * m);
#pragma unroll
      for (int c = 0; c < 3; ++c) l[c] *= kk;
    }
    // gamut, clamp, and back to a BT.709-coded signal
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = fmaf(t[6 + 3 * c + 2], l[2], fmaf(t[6 + 3 * c + 1], l[1], t[6 + 3 * c] * l[0]));
      v = fminf(fmaxf(v, 0.f), 1.f);
      const float w = v < 0.018053968510807f ? 4.5f * v : fmaf(1.09929682680944f, hdr_pow(v, 0.45f), -0.09929682680944f);
      o[c] = 255.f * w;
    }
    r = o[0], g = o[1], b = o[2];
  }

  __device__ __forceinline__ void operator()(f32x2 (&rgb)[3]) const {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float r = rgb[0][h], g = rgb[1][h], b = rgb[2][h];
      one(r, g, b);
      rgb[0][h] = r, rgb[1][h] = g, rgb[2][h] = b;
    }
  }
};

// The item of this workgroup, clamped into range before anything is addressed through it, as rs_item (pv_rs.h) does: its
// record, view and orientation, and the selected frame as (base, byte offset).  This file's own: the byte offset is formed
// inside the branch that tells the two kinds of source apart, and behind rs_item / rs_item_yuv, which multiply after it, all
// 40 kernels come out with that scalar multiply moved and other scalar registers (the same VGPR counts; profiles/r24/
// isa_vs_parent.md), which is not taken without the bit comparison and the timing on the device.
struct HdrItem {
  const pv_view_source* __restrict__ S;
  int view, orient;
  uintptr_t src;
  long frame_off;
};
__device__ __forceinline__ HdrItem hdr_item(const pv_batch_views_desc& d, int frames, int zi, int t) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  HdrItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  const int row = min(max(it->row, 0), d.n_rows - 1);
  const int ts = min(max(d.t_index[(long)row * d.t_stride + t], 0), r.S->N - 1);
  r.orient = r.S->orient & 7;
  if (frames) {   // read as constant memory: one scalar load (rs_item, pv_rs.h)
    typedef const uint64_t __attribute__((address_space(4))) * table_ptr;
    r.src = (uintptr_t) reinterpret_cast<table_ptr>(reinterpret_cast<uintptr_t>(r.S->src))[ts];
    r.frame_off = 0;
  } else {
    r.src = reinterpret_cast<uintptr_t>(r.S->src);
    r.frame_off = (long)ts * r.S->frame_stride;
  }
  return r;
}

template <int CSTEP> __device__ __forceinline__ RsYuvSrc hdr_src(const HdrItem& item) {
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = item.src;
  s.frame_off = item.frame_off;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  return s;
}

// CSTEP / FORM / D: as rs_strip_yuv; TRANSFER: PV_TRANSFER_PQ / PV_TRANSFER_HLG.  Items of upright records.
template <int CSTEP, int TRANSFER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void hdr_strip_kernel(const pv_batch_views_desc d, const RsItemLaunch g, const int frames,
                                                               const float* __restrict__ tone) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hs_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const HdrItem item = hdr_item(d, frames, zi, t);
  const RsYuvSrc s = hdr_src<CSTEP>(item);
  const HdrMap<TRANSFER> map(tone);
  rs_strip_yuv<CSTEP, FORM, D, unsigned short, HdrMap<TRANSFER>>(hs_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb,
                                                                 zi, t, true, map);
}

// The same for items of oriented records: the staged tile.
template <int CSTEP, int TRANSFER, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void hdr_tile_kernel(const pv_batch_views_desc d, const RsTileLaunch g, const int frames,
                                                              const float* __restrict__ tone) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ht_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const HdrItem item = hdr_item(d, frames, zi, t);
  const RsYuvSrc s = hdr_src<CSTEP>(item);
  const HdrMap<TRANSFER> map(tone);
  rs_tile_yuv<CSTEP, FORM, D, unsigned short, HdrMap<TRANSFER>>(ht_lds, g, s, item.orient, rs_dst(d, 3), d.yuv2rgb, zi, t, map);
}

// The transfer and the chroma arrangement in front of RS_DISPATCH; expects d, g, lds, stream, fr, tone and transfer in scope.
#define HDR_DISPATCH(GRID_X, KERNEL)                                                                                     \
  do {                                                                                                                   \
    if (transfer == PV_TRANSFER_PQ) {                                                                                    \
      if (d.c_step == 2) RS_DISPATCH(GRID_X, lds, (d, g, fr, tone), KERNEL, 2, PV_TRANSFER_PQ);                          \
      else RS_DISPATCH(GRID_X, lds, (d, g, fr, tone), KERNEL, 1, PV_TRANSFER_PQ);                                        \
    } else {                                                                                                             \
      if (d.c_step == 2) RS_DISPATCH(GRID_X, lds, (d, g, fr, tone), KERNEL, 2, PV_TRANSFER_HLG);                         \
      else RS_DISPATCH(GRID_X, lds, (d, g, fr, tone), KERNEL, 1, PV_TRANSFER_HLG);                                       \
    }                                                                                                                    \
  } while (0)

// What the wrapped entry point checks and sizes (rs_item_launch with its check of a record's `src`), then every run of
// upright / oriented items to the strip / tile kernels.
template <typename CheckSrc>
int hdr_run(const pv_hdr_views_desc& h, bool frames, const CheckSrc& check_src, pv_stream_t stream) {
  RsItemLaunch sg;
  RsTileLaunch tg;
  size_t lds_s, lds_t;
  if (int e = rs_item_launch(h.frames.batch, check_src, sg, lds_s, tg, lds_t)) return e;
  const int fr = frames ? 1 : 0, transfer = h.transfer;
  const float* tone = h.tone;
  auto upright = [&](const pv_batch_views_desc& d) -> int {
    const RsItemLaunch& g = sg;
    const size_t lds = lds_s;
    HDR_DISPATCH(pv_ceil_div(d.Ho, g.R), hdr_strip_kernel);
    PV_LAUNCH_CHECK();
    return PV_OK;
  };
  auto oriented = [&](const pv_batch_views_desc& d) -> int {
    const RsTileLaunch& g = tg;
    const size_t lds = lds_t;
    if (g.TR <= 0 || g.TC <= 0 || g.tiles_x <= 0) return PV_ERR_INVALID;   // not sized: no oriented item was announced
    HDR_DISPATCH(pv_ceil_div(d.Ho, g.TR) * g.tiles_x, hdr_tile_kernel);
    PV_LAUNCH_CHECK();
    return PV_OK;
  };
  return rs_item_runs(h.frames.batch, upright, oriented);
}

}  // namespace

extern "C" int pv_hdr_views(const pv_hdr_views_desc* hp, pv_stream_t stream) {
  if (!hp) return PV_ERR_INVALID;
  const pv_frame_views_desc& f = hp->frames;
  if (!hp->tone || hp->reserved != 0) return PV_ERR_INVALID;
  if (hp->transfer != PV_TRANSFER_PQ && hp->transfer != PV_TRANSFER_HLG) return PV_ERR_INVALID;
  // a 16-bit YUV 4:2:0 source is all this entry point carries
  return fv_with_table(f, [&](bool frames, const auto& check_src) { return hdr_run(*hp, frames, check_src, stream); },
                       f.batch.src_layout == PV_SRC_YUV420 && f.batch.src_dtype == PV_U16);
}
