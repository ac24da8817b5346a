// The resampling ingest: ten entry points in ten translation units.
//   pv_resample.hip   pv_resample_crop, pv_video_views    RGB / planar sources, one source per launch
//   pv_yuv.hip        pv_yuv_views, pv_yuv16_views        YUV 4:2:0 sources of 8- / 16-bit samples, one source per launch
//   pv_batch.hip      pv_batch_views                      either, one source per destination item
//   pv_frames.hip     pv_frame_views                      the same with every frame addressed through a pointer table
//   pv_frames16.hip   (launched from pv_frames.hip)       the 16-bit YUV kernels of pv_frame_views
//   pv_orient.hip     (launched from pv_batch.hip and pv_frames.hip)   the tile kernels of oriented records (orient != 0)
//   pv_hdr.hip        pv_hdr_views      pv_batch_views / pv_frame_views on 16-bit YUV with the PQ / HLG tap map
//   pv_region.hip     pv_region_views   a rectangle of the frame per destination frame, resized to the window
//   pv_area.hip       pv_area_views     a box filter (the windows of interpolate(mode="area")) in place of the blend: a staged-tile
//                                       body of its own (a window's rows are not two; its RGB body is in pv_area.h)
//   pv_packed.hip     (launched from pv_batch.hip, pv_frames.hip, pv_orient.hip, pv_region.hip and pv_area.hip)   the kernels of
//                                       packed-pixel launches (PV_SRC_BGR .. PV_SRC_ABGR): the RGB bodies with RsPacked<PB>
//   pv_yuv4.hip       (launched from the same five)       the kernels of YUV 4:2:2 / 4:4:4 launches (PV_SRC_YUV422, PV_SRC_YUV444):
//                                       the YUV bodies with the chroma shifts as a kernel argument (RsSub)
//   pv_yuyv.hip       (launched from the same five)       the kernels of packed YUV 4:2:2 launches (PV_SRC_YUYV422): the YUV bodies
//                                       with the macropixel arrangement (RsMacro)
// What they compute with is here, once: the pinned source coordinate, the destination forms with their stores, the taps and
// blends, the two staged-strip bodies (rs_strip_rgb, rs_strip_yuv: stage, barrier, gather) and the two staged-tile bodies of
// oriented records (rs_tile_rgb, rs_tile_yuv), the launch arithmetic (widest span, rows per strip, the LDS layout of a staged
// tile), the host-side checks of views, item range, destination and YUV planes, and the validation and sizing of an
// item-sourced launch (rs_item_launch).
// Around the bodies, every item-sourced kernel and entry point is made of the same pieces, each of them here once as well:
//   device  rs_item            the item of a workgroup: record, view, orientation and the selected frame, everything clamped
//           rs_item_rgb / rs_item_yuv   the geometry a body takes (RsRgbSrc / RsYuvSrc), filled from an item
//   host    RS_DISPATCH        the destination-form dispatch, grid and kernel arguments as parameters
//           RS_SOURCE_FORMS    the source-form dispatch in front of it
//           rs_walk_items      the walk over a launch's items: range, the record behind each, checked once per run
//           (fv_with_table, pv_frames.h: the optional pointer table in front of an entry point)
// The files keep what differs: the kernel wrappers (a __global__ function per body and source kind, two or three lines), what
// a rectangle or a tap map changes of the geometry, the validation of the one-source descriptors (rs_run, yuv_run), whose
// kernels fill the geometry from a by-value descriptor instead of a record, and the sizing that is an entry point's own.
// (Two device loaders are still apart, OvItem of pv_orient.hip and HdrItem of pv_hdr.hip: see rs_item.)
// Everything but RsItemLaunch, RsTileLaunch and pv_orient_launch is inline in an anonymous namespace: each translation unit
// keeps its own kernels.
#pragma once
#include <cstring>
#include <type_traits>
#include <vector>

#include "pv_common.h"

// What stays per launch of an item-sourced kernel (pv_batch.hip, pv_frames.hip, pv_frames16.hip): filled by rs_item_launch.
// It crosses translation units (pv_frame_yuv16_launch), so it is the one type here with external linkage.
struct RsItemLaunch {
  int32_t R;          // output rows per workgroup
  int32_t pitch;      // LDS bytes per staged (row, plane) -- YUV: per staged luma row; multiple of 16, >= 15 + widest span
  int32_t pitch_c;    // YUV: LDS bytes per staged chroma (row, plane)
  int32_t c_base;     // YUV: LDS offset of the chroma image: 2 R pitch
};

// What stays per launch of a tile kernel (pv_orient.hip: items of oriented records): filled by rs_tile_size.
struct RsTileLaunch {
  int32_t TR, TC;       // displayed rows x columns per workgroup; TC a multiple of 8
  int32_t tiles_x;      // tiles per window row
  int32_t rows, pitch;  // staged stored rows, LDS bytes per staged (row, plane) -- YUV: luma
  int32_t rows_c, pitch_c, c_base;   // YUV: staged chroma rows, LDS bytes per chroma (row, plane), LDS offset of the chroma image
};

// The tile kernels (pv_orient.hip) over the items of `d`, all of oriented records, on a launch rs_item_launch has validated
// and sized; frames: `src` of a record is a slice of the pointer table of pv_frame_views.
int pv_orient_launch(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream);

// The kernels of packed-pixel launches (pv_packed.hip: src_layout PV_SRC_BGR .. PV_SRC_ABGR), each on a launch its entry point
// has validated and sized: the strips of pv_batch_views / pv_frame_views, the tiles of their oriented records (called by
// pv_orient_launch) and the strips of pv_region_views (`regions`: its device copy); frames as above.
int pv_packed_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream);
int pv_packed_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream);
int pv_packed_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                      pv_stream_t stream);

// The kernels of YUV 4:2:2 / 4:4:4 launches (pv_yuv4.hip: src_layout PV_SRC_YUV422, PV_SRC_YUV444), each on a launch its entry
// point has validated and sized, as the packed ones above.
int pv_yuv4_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream);
int pv_yuv4_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream);
int pv_yuv4_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                    pv_stream_t stream);

// The kernels of packed YUV 4:2:2 launches (pv_yuyv.hip: src_layout PV_SRC_YUYV422), likewise.
int pv_yuyv_strips(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, pv_stream_t stream);
int pv_yuyv_tiles(const pv_batch_views_desc& d, bool frames, const RsTileLaunch& g, size_t lds, pv_stream_t stream);
int pv_yuyv_regions(const pv_batch_views_desc& d, bool frames, const RsItemLaunch& g, size_t lds, const pv_view_region* regions,
                    pv_stream_t stream);

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsMaxRows = 8;            // output rows per workgroup
constexpr int kRsLdsBudget = 32 * 1024;  // staging bytes per workgroup: 4-5 workgroups per CU (160 KiB)
constexpr int kRsLdsMax = 64 * 1024;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

enum { RS_C4 = 0, RS_CL = 1, RS_PLANAR = 2 };

// Source coordinate of destination index d (the pinned formula: every operation rounded on its own, no contraction, so
// that the host, which sizes the LDS span, and every thread agree on i0 / i1).
__host__ __device__ __forceinline__ void rs_coord(float s, int d, int n_in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  const float a = (float)d + 0.5f;
  const float m = s * a;
  float r = m - 0.5f;
  r = r < 0.f ? 0.f : r;
  i0 = (int)r;
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;   // r < n_in - 0.5 for every d inside the scaled frame; this keeps reads in bounds regardless
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = r - (float)i0;
}

// The box filter's window of destination index d (pv_area_views: the pinned integer formula, the windows of
// F.interpolate(mode="area")): source indices [start, end).  d < n_out and n_in * n_out <= 2^24 on a validated launch, so the
// products fit 32 bits and 0 <= start < end <= n_in; the clamps keep a device copy that is not the validated one in bounds.
__host__ __device__ __forceinline__ void rs_area_win(int d, int n_in, int n_out, int& start, int& end) {
  n_out = n_out > 0 ? n_out : 1;
  start = (d * n_in) / n_out;
  end = ((d + 1) * n_in + n_out - 1) / n_out;
  start = start < 0 ? 0 : (start < n_in - 1 ? start : n_in - 1);
  end = end > n_in ? n_in : end;
  end = end > start ? end : start + 1;
}

template <typename D> struct RsVec;   // one 16-byte store of G = 16 / sizeof(D) elements
template <> struct RsVec<bf16_t> {
  static constexpr int G = 8;
  static __device__ __forceinline__ void store(bf16_t* p, const float* f) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)f[i];
    *reinterpret_cast<bf16x8*>(p) = v;
  }
};
template <> struct RsVec<float> {
  static constexpr int G = 4;
  static __device__ __forceinline__ void store(float* p, const float* f) {
    *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
  }
};

template <int FORM, typename D> struct RsGroup { static constexpr int G = FORM == RS_PLANAR ? RsVec<D>::G : (FORM == RS_C4 ? 2 : 1); };

// The epilogue of a gather thread: out[c][j] is channel c of output pixel (y, x0 + j) of frame t of destination item zi,
// already through the affine map (pad channels zero); the first `nvalid` of the G pixels lie inside the row.  One
// rounding to D; 16-byte stores where the group is whole and aligned, element by element otherwise.
template <int FORM, typename D, int G>
__device__ __forceinline__ void rs_store_group(void* dst, const float (&out)[4][G], int C, int T, int Ho, int Wo, int c_p,
                                               int ld, int64_t bs, int zi, int t, int y, int x0, int nvalid) {
  if constexpr (FORM == RS_PLANAR) {
    const long HW = (long)Ho * Wo;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        D* p = static_cast<D*>(dst) + (((long)zi * C + c) * T + t) * HW + (long)y * Wo + x0;
        if (nvalid == G && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
          RsVec<D>::store(p, out[c]);
        } else {
#pragma unroll
          for (int j = 0; j < G; ++j)
            if (j < nvalid) p[j] = (D)out[c][j];
        }
      }
    }
  } else if constexpr (FORM == RS_C4) {
    bf16_t* p = static_cast<bf16_t*>(dst) + (long)zi * bs + ((((long)t * Ho + y) * Wo) + x0) * 4;
    if (nvalid == G && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
      for (int j = 0; j < G; j += 2) {           // two voxels = one 16-byte chunk of the first-layer layout
        const bf16x8 o = {(bf16_t)out[0][j], (bf16_t)out[1][j], (bf16_t)out[2][j], (bf16_t)out[3][j],
                          (bf16_t)out[0][j + 1], (bf16_t)out[1][j + 1], (bf16_t)out[2][j + 1], (bf16_t)out[3][j + 1]};
        *reinterpret_cast<bf16x8*>(p + j * 4) = o;
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (j < nvalid) {
          const bf16x4 o = {(bf16_t)out[0][j], (bf16_t)out[1][j], (bf16_t)out[2][j], (bf16_t)out[3][j]};
          *reinterpret_cast<bf16x4*>(p + j * 4) = o;
        }
    }
  } else {
    D* p = static_cast<D*>(dst) + (long)zi * bs + ((((long)t * Ho + y) * Wo) + x0) * ld;
    const float f[8] = {out[0][0], out[1][0], out[2][0], out[3][0], 0.f, 0.f, 0.f, 0.f};
    Chunk8<D> o;
    o.from_f32(f);
    o.store(p);
    o.zero();
    for (int k = 8; k < c_p; k += 8) o.store(p + k);
  }
}

// ---- taps and blends ------------------------------------------------------------------------------------------------
// One tap of a staged RGB / planar row, in the source dtype.
template <typename S> __device__ __forceinline__ float rs_tap(const unsigned char* lds, int off);
template <> __device__ __forceinline__ float rs_tap<unsigned char>(const unsigned char* lds, int off) { return (float)lds[off]; }
template <> __device__ __forceinline__ float rs_tap<float>(const unsigned char* lds, int off) {
  return *reinterpret_cast<const float*>(lds + off);
}

__device__ __forceinline__ f32x2 yuv_splat(float v) { return f32x2{v, v}; }

// One staged YUV sample at LDS byte offset `off`, read whole and unsigned: a byte, or a 16-bit little-endian code (the
// offset is then even: the entry points refuse odd source addresses, and the LDS image keeps a row's `addr & 15`).
template <typename SMP> __device__ __forceinline__ float yuv_sample(const unsigned char* lds, int off) {
  if constexpr (sizeof(SMP) == 1) return (float)lds[off];
  else return (float)*reinterpret_cast<const unsigned short*>(lds + off);
}

// The tap map: what a YUV body does to a converted, clamped tap before the blend.  RsTapNone, the default, is nothing: the
// tap enters the blend as it is (pv_yuv_views' rule).  Any other type is a callable over the pair of taps yuv_tap2 makes,
// void operator()(f32x2 (&rgb)[3]) const, workgroup-uniform state in registers (pv_hdr.hip: the PQ / HLG to SDR map).
struct RsTapNone { static constexpr bool kNone = true; };

// Two taps of the virtual RGB frame -- the same column of the two source rows -- as packed fp32 pairs (v_pk_fma_f32 does
// both for the price of one): per channel three fused multiply-adds in the header's order, then the clamp, then the tap map.
template <typename SMP = unsigned char, typename MAP = RsTapNone>
__device__ __forceinline__ void yuv_tap2(const float (&m)[12], const unsigned char* lds, int oy0, int ou0, int ov0, int oy1, int ou1,
                                         int ov1, f32x2 (&rgb)[3], const MAP& map = MAP()) {
  const f32x2 Y = {yuv_sample<SMP>(lds, oy0), yuv_sample<SMP>(lds, oy1)}, U = {yuv_sample<SMP>(lds, ou0), yuv_sample<SMP>(lds, ou1)},
              V = {yuv_sample<SMP>(lds, ov0), yuv_sample<SMP>(lds, ov1)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const f32x2 v = __builtin_elementwise_fma(yuv_splat(m[c * 4 + 2]), V, __builtin_elementwise_fma(yuv_splat(m[c * 4 + 1]), U,
                        __builtin_elementwise_fma(yuv_splat(m[c * 4]), Y, yuv_splat(m[c * 4 + 3]))));
    rgb[c] = f32x2{fminf(fmaxf(v[0], 0.f), 255.f), fminf(fmaxf(v[1], 0.f), 255.f)};
  }
  if constexpr (!MAP::kNone) map(rgb);
}

// The pinned blend and the affine map with the contraction spelled out, so that every instantiation gives the same bits:
// p0 / p1 hold column i0x / i1x of the rows (i0y, i1y); h = {top, bottom} = lx1 p1 + (lx0 p0), v = ly1 bottom + (ly0 top).
__device__ __forceinline__ float yuv_blend(float ly0, float ly1, float lx0, float lx1, f32x2 p0, f32x2 p1, float sc, float sh) {
#pragma clang fp contract(off)
  const f32x2 h = __builtin_elementwise_fma(yuv_splat(lx1), p1, yuv_splat(lx0) * p0);
  const float v = fmaf(ly1, h[1], ly0 * h[0]);
  return fmaf(v, sc, sh);
}

// ---- the staged strip ---------------------------------------------------------------------------------------------
// A bandwidth-bound gather.  One workgroup owns a strip of R output rows (blockIdx.x) of one destination frame t of one
// destination item zi:
//   1. stage: the source span those rows need -- per output row the two source rows i0y, i1y (or, when the strip's source
//      rows are at most 2R, as in upscaling, that contiguous run of rows once), columns [i0x(first), i1x(last)] -- is
//      copied to LDS in the SOURCE dtype with aligned 16-byte global loads, a batch of four per thread, and 16-byte LDS
//      writes.  YUV stages the luma span and the chroma span behind it: chroma rows (y >> 1) of the same rows, columns
//      [xs0 >> 1, xs1 >> 1]; in the contiguous case every chroma row once, so half as many as luma rows (4:2:0; the shifts are
//      the layout's -- RsSub -- and full-height chroma stages as many chroma rows as luma rows, at most 2R).  A row of a span
//      may start at any byte address (Ws = 340 gives 4-byte-aligned rows, an odd Ws, a pitched surface, an odd base or the
//      +1 of the second interleaved sample none at all): the loads fetch the aligned 16-byte granules that cover the span,
//      and the LDS image of each row keeps the span's offset inside its first granule (`addr & 15`), so unaligned rows cost
//      nothing extra.  A granule that covers a byte of the span lies in the same page as that byte, so the up to 15 bytes
//      fetched in front of and behind the span are never used and never fault.
//   2. gather: a thread owns G x-adjacent output pixels of one row (G = one 16-byte store per channel row for planar
//      destinations, 2 = one 16-byte chunk for the 4-channel layout, 1 voxel for channels-last), takes its 4 taps per
//      channel from LDS (YUV: the four Y taps and the (U, V) pair behind each, converted and clamped per tap), blends in
//      fp32, applies the affine map and hands the group to rs_store_group.  Groups cut by the right edge (Wo not a multiple
//      of G) or not 16-byte aligned in the destination (odd Wo) are stored element by element.  (Eight pixels per thread
//      for the 4-channel layout -- four 16-byte stores 64 bytes apart, as ingest_c4_vec8_kernel does -- measured up to 17 %
//      slower here: DESIGN.md 4.6.)
// The launch sizes R and the LDS pitch(es) of a staged row; the geometry is a struct of workgroup-uniform scalars that the
// kernel fills from its descriptor or from the item's record.  The view's window origin arrives selected (rs_view_off):
// a runtime index into a by-value descriptor would put the descriptor in scratch.  check_span: the source is a per-item
// record, which the launch may not have been sized for; a workgroup whose span exceeds the pitch then stages nothing and
// writes nothing.  The host sizes a one-source launch from the very values the kernel sees, so those kernels skip the test.

// What the gather writes, and the affine map in front of the store.
struct RsDst {
  void* dst;
  int C, T, Ho, Wo, c_p, ld;
  int64_t bs;
  const float* ch_scale;
  const float* ch_shift;
};
template <typename Desc> __device__ __forceinline__ RsDst rs_dst(const Desc& d, int C) {
  return RsDst{d.dst, C, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, d.ch_scale, d.ch_shift};
}

// Selected, not indexed -- and from values the caller has loaded, not through a reference to the three: the compiler keeps
// conditional loads as branches.
__device__ __forceinline__ int rs_view_off(int view, int off0, int off1, int off2) {
  return view == 0 ? off0 : (view == 1 ? off1 : off2);
}

// An RGB / planar source: clip `clip_frame0 / (planes * N)` of [.., C, N, Hs, Ws] or [.., N, Hs, Ws, 3].
struct RsRgbSrc {
  static constexpr bool kWindow = false;
  uintptr_t src;
  int Hs, Ws, N;        // N: frames per source plane, which is the plane stride in frames
  float sy, sx;         // (float)Hs / (float)Hn, (float)Ws / (float)Wn: divided once, on the host
  int yoff, xoff;       // the view's window origin inside Hn x Wn
  int ts;               // the selected frame, clamped into [0, N - 1] before any address is formed
  long clip_frame0;     // frames from `src` to frame 0 of the clip
};

// The same with a RECTANGLE of every frame as the source (pv_region.hip): Hs x Ws, what the coordinates are clamped with, are
// the rectangle's, and the stored frame keeps an extent of its own, which the row and frame strides follow.
struct RsRgbWin : RsRgbSrc {
  static constexpr bool kWindow = true;
  int Hf, Wf;           // the stored frame
  int top, left;        // the rectangle's origin in it: rows [top, top + Hs) x columns [left, left + Ws)
};

// A PACKED source (PV_SRC_BGR .. PV_SRC_ABGR, include/pv_mi355x.h "packed pixels"): a frame-interleaved uint8 source whose
// pixel has PB = 3 or 4 bytes, R, G and B at bytes o[0..2] of it -- workgroup-uniform, so they stay in scalar registers and one
// kernel serves every channel order of its pixel size --, rows at the record's pitch and frames at its stride (a dense source
// derives both from Ws and Hs).  The bodies take it behind a last template parameter whose default, RsDense, leaves every other
// kernel of the ingest with the instructions it had.  PB == 4: a pixel is one aligned dword of the source (the entry points
// refuse anything else) and of its LDS image, which keeps a row's `addr & 15`: a tap is ONE dword LDS read (rs_px4) and the
// channels are bytes of the register (rs_px4_ch); the fourth byte never enters a value.  PB == 3 reads bytes, as [.., 3] does.
struct RsDense { static constexpr bool kPacked = false; static constexpr int PB = 0; };
template <int PB_> struct RsPacked {
  static constexpr bool kPacked = true;
  static constexpr int PB = PB_;
  int o[3];                   // byte of R, G, B inside a pixel
  long row_bytes, frame_bytes;
};
struct RsPackedArg { int32_t r, g, b; };   // the kernel argument behind o[]
// R, G, B byte offsets and the pixel size of a packed src_layout (0: not a packed layout).
inline int rs_packed_px(int src_layout, RsPackedArg* o = nullptr) {
  static const int8_t at[5][4] = {{2, 1, 0, 3}, {0, 1, 2, 4}, {2, 1, 0, 4}, {1, 2, 3, 4}, {3, 2, 1, 4}};   // BGR RGBA BGRA ARGB ABGR
  if (src_layout < PV_SRC_BGR || src_layout > PV_SRC_ABGR) return 0;
  const int8_t* a = at[src_layout - PV_SRC_BGR];
  if (o) *o = RsPackedArg{a[0], a[1], a[2]};
  return a[3];
}
template <int PB> __device__ __forceinline__ RsPacked<PB> rs_item_packed(const pv_view_source* __restrict__ V, const RsPackedArg& o) {
  return RsPacked<PB>{{o.r, o.g, o.b}, (long)V->y_pitch, (long)V->frame_stride};
}
// The byte of channel c behind the LDS offset of a pixel: c for [.., 3], the record's order for 3-byte pixels, none for dwords.
template <typename PK> __device__ __forceinline__ int rs_ch_byte(const PK& pk, int c) {
  if constexpr (!PK::kPacked) return c;
  else if constexpr (PK::PB == 4) return 0;
  else return pk.o[c < 3 ? c : 0];
}
__device__ __forceinline__ unsigned rs_px4(const unsigned char* lds, int off) { return *reinterpret_cast<const unsigned*>(lds + off); }
__device__ __forceinline__ float rs_px4_ch(unsigned w, int byte) { return (float)((w >> (8 * byte)) & 0xffu); }
// The four taps of channel c of a packed pixel quad: bytes of the four dwords (PB == 4) or four byte reads at the channel's offset.
template <typename PK>
__device__ __forceinline__ void rs_packed_taps(const PK& pk, const unsigned char* lds, const int (&at)[4], const unsigned (&w)[4], int c,
                                               float (&p)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (PK::PB == 4) p[k] = rs_px4_ch(w[k], pk.o[c]);
    else p[k] = (float)lds[at[k] + pk.o[c]];
  }
}
// The blend and the affine map of the RGB bodies,
//   v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11),  out = v * sc + sh,
// with the contraction spelled out as the compiler forms it in every dense instantiation (profiles/r26/isa_vs_parent.md): left
// to the compiler, the packed instantiations fuse the other product of each sum and differ in the last bit of an fp32 output.
__device__ __forceinline__ float rs_blend_rgb(float ly0, float ly1, float lx0, float lx1, const float (&p)[4], float sc, float sh) {
#pragma clang fp contract(off)
  const float h0 = fmaf(lx0, p[0], lx1 * p[1]), h1 = fmaf(lx0, p[2], lx1 * p[3]);   // p: (row 0, row 1) x (column i0x, i1x)
  return fmaf(fmaf(ly0, h0, ly1 * h1), sc, sh);
}

// S: source element (unsigned char | float); INTER: frame-interleaved [.., Hs, Ws, 3] source; FORM / D: destination.
// SRC: RsRgbSrc, or RsRgbWin for a rectangle of the stored frame (deduced; the default keeps today's expressions).
// PK: RsDense, or RsPacked<PB> for packed pixels (INTER, bytes, three channels; deduced from the last argument).
template <typename S, bool INTER, int FORM, typename D, typename SRC = RsRgbSrc, typename PK = RsDense>
__device__ __forceinline__ void rs_strip_rgb(unsigned char* lds, int R, int pitch, const SRC& s, const RsDst& d, int zi, int t,
                                             bool check_span, const PK& pk = PK()) {
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int XB = PK::kPacked ? PK::PB : (INTER ? 3 : (int)sizeof(S));   // bytes from one source column to the next
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);
  const int planes = INTER ? 1 : d.C;

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(s.sx, s.xoff, s.Ws, xs0, unused, lunused);
  rs_coord(s.sx, s.xoff + d.Wo - 1, s.Ws, unused, xs1, lunused);
  rs_coord(s.sy, s.yoff + row0, s.Hs, ybase, unused, lunused);
  rs_coord(s.sy, s.yoff + row0 + nrows - 1, s.Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int span_bytes = (xs1 - xs0 + 1) * XB;
  if (check_span && span_bytes + 15 > pitch) return;

  // byte address of column xs0 of source row y of plane `pl` of the selected frame
  long row_bytes, frame_bytes, first;
  if constexpr (PK::kPacked) {                     // the record's pitch and stride; a rectangle's origin in the first address
    row_bytes = pk.row_bytes;
    frame_bytes = pk.frame_bytes;
    first = (s.clip_frame0 + s.ts) * frame_bytes + (long)xs0 * XB;
    if constexpr (SRC::kWindow) first += (long)s.top * row_bytes + (long)s.left * XB;
  } else if constexpr (SRC::kWindow) {             // strides of the stored frame, the rectangle's origin in the first address
    row_bytes = (long)s.Wf * XB;
    frame_bytes = (long)s.Hf * row_bytes;
    first = (s.clip_frame0 + s.ts) * frame_bytes + (long)s.top * row_bytes + (long)(s.left + xs0) * XB;
  } else {
    row_bytes = (long)s.Ws * XB;
    frame_bytes = (long)s.Hs * row_bytes;
    first = (s.clip_frame0 + s.ts) * frame_bytes + (long)xs0 * XB;
  }
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
        int y = ybase + slot;
        if (!dense) {
          int i0, i1;
          rs_coord(s.sy, s.yoff + row0 + (slot >> 1), s.Hs, i0, i1, lunused);
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
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
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
    rs_coord(s.sy, s.yoff + y, s.Hs, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int s0 = dense ? i0y - ybase : 2 * r, s1 = dense ? i1y - ybase : 2 * r + 1;
    int ro0[4], ro1[4];                            // LDS byte offset of column xs0, channel c, in the two source rows
    int pb0 = 0, pb1 = 0;                          // packed pixels: of the pixel itself
    if constexpr (PK::kPacked) pb0 = s0 * pitch + (int)(row_addr(i0y, 0) & 15), pb1 = s1 * pitch + (int)(row_addr(i1y, 0) & 15);
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
      rs_coord(s.sx, s.xoff + x, s.Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = (i0x - xs0) * XB, o1 = (i1x - xs0) * XB;
      if constexpr (PK::kPacked) {                 // PB == 4: four dword reads, the channels out of the registers
        const int at[4] = {pb0 + o0, pb0 + o1, pb1 + o0, pb1 + o1};
        unsigned w[4] = {0, 0, 0, 0};
        if constexpr (PK::PB == 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = rs_px4(lds, at[k]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float p[4];
          rs_packed_taps(pk, lds, at, w, c, p);
          out[c][j] = rs_blend_rgb(ly0, ly1, lx0, lx1, p, sc[c], sh[c]);
        }
        out[3][j] = 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < d.C) {
            const float p00 = rs_tap<S>(lds, ro0[c] + o0), p01 = rs_tap<S>(lds, ro0[c] + o1);
            const float p10 = rs_tap<S>(lds, ro1[c] + o0), p11 = rs_tap<S>(lds, ro1[c] + o1);
            const float v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
            out[c][j] = v * sc[c] + sh[c];
          } else {
            out[c][j] = 0.f;
          }
        }
      }
      // packed pixels: finish this pixel before the next one starts (as in rs_strip_yuv: 134 -> 70 VGPRs for G = 8)
      if constexpr (PK::kPacked) asm volatile("" : "+v"(out[0][j]), "+v"(out[1][j]), "+v"(out[2][j]));
    }
    const int x0 = gx * G;
    const int nvalid = min(G, d.Wo - x0);
    rs_store_group<FORM, D, G>(d.dst, out, d.C, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, nvalid);
  }
}

// The chroma subsampling of a YUV launch: the chroma sample of luma pixel (y, x) is (y >> csy, x >> csx).  The YUV bodies take
// it behind a last template parameter whose default, RsSub420, is the constant pair (1, 1) and leaves every 4:2:0 kernel with
// the instructions it had.  RsSub is the pair as a by-value kernel argument (PV_SRC_YUV422: (0, 1), PV_SRC_YUV444: (0, 0);
// include/pv_mi355x.h, "YUV 4:2:2 and 4:4:4") -- uniform over the launch and held in scalar registers, so one kernel of
// pv_yuv4.hip serves both layouts, as RsPackedArg serves every channel order.
// (Static constants, not functions: `y >> sub.csy` is then the literal `y >> 1` from the front end on, and the 4:2:0 kernels
// come out instruction for instruction as they were; behind a constexpr member function they did not -- profiles/r27.)
struct RsSub420 { static constexpr int csy = 1, csx = 1; };
struct RsSub { int32_t csy, csx; };
// The shifts of a YUV src_layout; false: not a YUV layout.
inline bool rs_yuv_sub(int src_layout, RsSub* c = nullptr) {
  const bool yuv = src_layout == PV_SRC_YUV420 || src_layout == PV_SRC_YUV422 || src_layout == PV_SRC_YUV444 ||
                   src_layout == PV_SRC_YUYV422;   // packed 4:2:2 subsamples as PV_SRC_YUV422 does
  if (yuv && c) *c = RsSub{src_layout == PV_SRC_YUV420 ? 1 : 0, src_layout == PV_SRC_YUV444 ? 0 : 1};
  return yuv;
}
// The layouts whose kernels are in pv_yuv4.hip.
inline bool rs_yuv4(int src_layout) { return src_layout == PV_SRC_YUV422 || src_layout == PV_SRC_YUV444; }

// The sample arrangement of a YUV launch, the last template parameter of the YUV bodies.  RsPlanes, the default, is a luma
// image and a chroma image behind it (every layout but one) and leaves each of those kernels with the instructions it had.
// RsMacro is PACKED 4:2:2 (PV_SRC_YUYV422; include/pv_mi355x.h, "packed YUV 4:2:2"; the kernels are in pv_yuyv.hip): ONE plane
// whose row is Ws / 2 macropixels of four samples -- two luma, one U, one V, in the record's order -- so a source row is staged
// once and serves as both images.  What changes in a body, and nothing else:
//   the staged span of a row is that of the macropixels [xs0 >> 1, xs1 >> 1], CB = 4 SB bytes each (CSTEP is 4), at pitch_y;
//   no chroma row is staged: pitch_c and c_base are unused;
//   luma column i is at y_byte + (i - x_first) * 2 SB of its staged row, x_first = xs0 & ~1 the column the span starts at,
//   and its U / V sample at u_byte / v_byte + ((i >> 1) - (x_first >> 1)) * CB of THE SAME row.
// u_byte / v_byte are the record's offsets inside a macropixel (RsYuvSrc; c_off_a = c_off_b = 0) and luma takes the other two
// samples: y_byte is 0 where U and V are the odd samples (YUY2, YVYU) and SB where they are the even ones (UYVY, VYUY).  The
// subsampling is the constant pair RsSub422.  (A static constant, as RsSub420's: see there.)
struct RsPlanes { static constexpr bool kMacro = false; };
struct RsMacro { static constexpr bool kMacro = true; };
struct RsSub422 { static constexpr int csy = 0, csx = 1; };
// The layout whose kernels are in pv_yuyv.hip.
inline bool rs_yuyv(int src_layout) { return src_layout == PV_SRC_YUYV422; }
// Byte of the first luma sample of a macropixel whose U sample is at u_byte.
template <int SB> __host__ __device__ __forceinline__ int rs_macro_y_byte(int u_byte) { return (u_byte & SB) ? 0 : SB; }

// A YUV source: the planes of the selected frame.
struct RsYuvSrc {
  uintptr_t src;
  long frame_off;           // bytes from `src` to the selected frame, its index clamped before the product
  int Hs, Ws;
  float sy, sx;             // as in RsRgbSrc
  int yoff, xoff;
  int y_pitch, c_pitch;     // bytes per luma / chroma row of the source
  long c_off_a, c_off_b;    // byte offset inside a frame of staged chroma plane 0 / 1 (c_step 2: only plane 0, min(u, v))
  int u_byte, v_byte;       // c_step 2: the byte offset of U / V inside an interleaved pair (0 or one sample); c_step 1: 0
};
// The staged chroma planes behind a frame's u_offset / v_offset; `inter`: c_step 2.
__host__ __device__ __forceinline__ void rs_chroma_planes(bool inter, int64_t u_off, int64_t v_off, RsYuvSrc& s) {
  const int64_t c_min = u_off < v_off ? u_off : v_off;
  s.c_off_a = inter ? c_min : u_off;
  s.c_off_b = inter ? c_min : v_off;
  s.u_byte = inter ? (int)(u_off - c_min) : 0;
  s.v_byte = inter ? (int)(v_off - c_min) : 0;
}

// CSTEP: samples between x-adjacent samples of one chroma plane (2: U and V interleaved in ONE staged plane; 1: two planes).
// pitch_y / pitch_c: LDS bytes per staged luma row / chroma (row, plane); c_base: LDS offset of the chroma image.
// SMP: the sample, unsigned char or unsigned short (16-bit little-endian codes: P010 / yuv420p10le and their 12- and 16-bit
// kin).  Spans, source addresses and LDS offsets count SB = sizeof(SMP) bytes per luma column and CSTEP * SB per chroma
// column; pitches and plane offsets are bytes in either case.  Two-byte samples need even source addresses (checked on the
// host: rs_check_yuv16_even), which makes every 16-bit LDS read naturally aligned.  MAP: the tap map (RsTapNone: none).
// SUB: the chroma subsampling (RsSub420, or RsSub for the 4:2:2 / 4:4:4 kernels of pv_yuv4.hip; deduced from the last argument).
// ARR: the sample arrangement (RsPlanes, or RsMacro for the packed 4:2:2 kernels of pv_yuyv.hip, with CSTEP 4 and RsSub422).
template <int CSTEP, int FORM, typename D, typename SMP = unsigned char, typename MAP = RsTapNone, typename SUB = RsSub420,
          typename ARR = RsPlanes>
__device__ __forceinline__ void rs_strip_yuv(unsigned char* lds, int R, int pitch_y, int pitch_c, int c_base, const RsYuvSrc& s,
                                             const RsDst& d, const float* yuv2rgb, int zi, int t, bool check_span,
                                             const MAP& map = MAP(), const SUB& sub = SUB()) {
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int CP = CSTEP == 1 ? 2 : 1;           // staged chroma planes
  constexpr int SB = (int)sizeof(SMP);             // bytes from one luma column to the next
  constexpr int CB = CSTEP * SB;                   // bytes from one chroma column to the next
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, d.Ho - row0);

  int xs0, xs1, ybase, ylast, unused;
  float lunused;
  rs_coord(s.sx, s.xoff, s.Ws, xs0, unused, lunused);
  rs_coord(s.sx, s.xoff + d.Wo - 1, s.Ws, unused, xs1, lunused);
  rs_coord(s.sy, s.yoff + row0, s.Hs, ybase, unused, lunused);
  rs_coord(s.sy, s.yoff + row0 + nrows - 1, s.Hs, unused, ylast, lunused);
  const bool dense = ylast - ybase + 1 <= 2 * R;   // the strip's source rows fit the 2R slots as one contiguous run
  const int nslots = dense ? ylast - ybase + 1 : 2 * nrows;
  const int cxs0 = xs0 >> sub.csx, cybase = ybase >> sub.csy;
  const int ncslots = ARR::kMacro ? 0 : (dense ? (ylast >> sub.csy) - cybase + 1 : 2 * nrows);   // dense: <= R + 1 (4:2:0), <= 2R (full-height chroma)
  const int span_y = ARR::kMacro ? ((xs1 >> 1) - cxs0 + 1) * CB : (xs1 - xs0 + 1) * SB;   // macropixels: one staged row, the span of both
  const int span_c = ((xs1 >> sub.csx) - cxs0 + 1) * CB;
  if (check_span && (span_y + 15 > pitch_y || (!ARR::kMacro && span_c + 15 > pitch_c))) return;

  const uintptr_t frame = s.src + s.frame_off;
  // the first staged byte of source row y: luma column xs0, or the macropixel that holds it
  auto y_addr = [&](int y) -> uintptr_t { return frame + (long)y * s.y_pitch + (ARR::kMacro ? cxs0 * CB : xs0 * SB); };
  auto c_addr = [&](int cy, int pl) -> uintptr_t {
    return frame + (pl == 0 ? s.c_off_a : s.c_off_b) + (long)cy * s.c_pitch + (long)cxs0 * CB;
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
        int y = ybase + slot, cy = cybase + slot;
        if (!dense) {
          int i0, i1;
          rs_coord(s.sy, s.yoff + row0 + (slot >> 1), s.Hs, i0, i1, lunused);
          y = (slot & 1) ? i1 : i0;
          cy = y >> sub.csy;
        }
        const uintptr_t a = luma ? y_addr(y) : c_addr(cy, pl);
        if (ch * 16 < (int)(a & 15) + (luma ? span_y : span_c)) {
          val[u] = *reinterpret_cast<const u32x4*>((a & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = (luma ? sp * pitch_y : c_base + sp * pitch_c) + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- gather ------------------------------------------------------------------------------------------------
  float m[12], sc[3], sh[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = yuv2rgb[i];
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
    rs_coord(s.sy, s.yoff + y, s.Hs, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int s0 = dense ? i0y - ybase : 2 * r, s1 = dense ? i1y - ybase : 2 * r + 1;
    const int cs0 = dense ? (i0y >> sub.csy) - cybase : 2 * r, cs1 = dense ? (i1y >> sub.csy) - cybase : 2 * r + 1;
    // LDS byte offset of column xs0 (luma) / cxs0 (U, V) in the two source rows
    int yo0 = s0 * pitch_y + (int)(y_addr(i0y) & 15), yo1 = s1 * pitch_y + (int)(y_addr(i1y) & 15);
    int uo0, uo1, vo0, vo1;
    if constexpr (ARR::kMacro) {                   // the staged row is the chroma row: U, V and luma at their bytes of a macropixel
      uo0 = yo0 + s.u_byte, uo1 = yo1 + s.u_byte, vo0 = yo0 + s.v_byte, vo1 = yo1 + s.v_byte;
      yo0 += rs_macro_y_byte<SB>(s.u_byte), yo1 += rs_macro_y_byte<SB>(s.u_byte);
    } else {
      uo0 = c_base + cs0 * CP * pitch_c + (int)(c_addr(i0y >> sub.csy, 0) & 15) + s.u_byte;
      uo1 = c_base + cs1 * CP * pitch_c + (int)(c_addr(i1y >> sub.csy, 0) & 15) + s.u_byte;
      vo0 = c_base + (cs0 * CP + CP - 1) * pitch_c + (int)(c_addr(i0y >> sub.csy, CP - 1) & 15) + s.v_byte;
      vo1 = c_base + (cs1 * CP + CP - 1) * pitch_c + (int)(c_addr(i1y >> sub.csy, CP - 1) & 15) + s.v_byte;
    }
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(gx * G + j, d.Wo - 1);     // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(s.sx, s.xoff + x, s.Ws, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      const int o0 = ARR::kMacro ? (i0x - 2 * cxs0) * 2 * SB : (i0x - xs0) * SB;   // macropixels: luma columns are 2 SB apart
      const int o1 = ARR::kMacro ? (i1x - 2 * cxs0) * 2 * SB : (i1x - xs0) * SB;
      const int c0 = ((i0x >> sub.csx) - cxs0) * CB, c1 = ((i1x >> sub.csx) - cxs0) * CB;
      f32x2 p0[3], p1[3];                          // {row i0y, row i1y} of column i0x / i1x, per channel
      yuv_tap2<SMP, MAP>(m, lds, yo0 + o0, uo0 + c0, vo0 + c0, yo1 + o0, uo1 + c0, vo1 + c0, p0, map);
      yuv_tap2<SMP, MAP>(m, lds, yo0 + o1, uo0 + c1, vo0 + c1, yo1 + o1, uo1 + c1, vo1 + c1, p1, map);
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

// ---- the staged tile: oriented records ---------------------------------------------------------------------------------
// A record with orient != 0 (include/pv_mi355x.h: rot | mirror << 2) is resampled ON ITS DISPLAYED FRAME D: rs_coord runs on
// Hd x Wd, and a tap at displayed (y, x) is stored pixel (r, c) = (r0 + ry y + rx x, c0 + cy y + cx x), one of y / x per
// coordinate (rs_orient_map).  For rot & 1 an output row is a source COLUMN, so the strip's whole-row spans would degenerate
// to a few bytes per staged row; the bodies below own a TILE instead: TR displayed rows x TC displayed columns (blockIdx.x,
// row-major over the window) of one frame of one item.
//   1. stage: the displayed rows / columns the tile's taps touch are contiguous ranges, and the map is monotone in each, so
//      the stored footprint is one rectangle [sr0, sr1] x [sc0, sc1].  Its rows are copied to LDS in the source dtype as
//      the strip copies a contiguous run: the aligned 16-byte granules that cover each row's span, the LDS image keeping the
//      span's `addr & 15`.  YUV stages the chroma rectangle [sr0 >> 1, sr1 >> 1] x [sc0 >> 1, sc1 >> 1] behind the luma one.
//      A square-ish tile keeps the staged rows of a transposing record several granules long.
//   2. one barrier.
//   3. gather: as in the strip a thread owns G x-adjacent displayed pixels of one row -- TC is a multiple of 8, so a group
//      starts where the strip's groups start -- takes its taps from LDS through the map, every stored coordinate clamped
//      into the staged rectangle, blends with the strip's own expressions and hands the group to rs_store_group.
// The host sizes TR, TC, the staged rows and the LDS pitch(es) from the widest footprint over the records the launch's
// oriented items name (rs_tile_size); a workgroup whose footprint exceeds them stages nothing and writes nothing.
struct RsOrient { int r0, ry, rx, c0, cy, cx; };
__host__ __device__ __forceinline__ RsOrient rs_orient_map(int orient, int Hs, int Ws) {
  const int rot = orient & 3;
  const int Wd = (rot & 1) ? Hs : Ws;
  const int m0 = (orient & 4) ? Wd - 1 : 0, mx = (orient & 4) ? -1 : 1;   // x' = m0 + mx x
  if (rot == 0) return RsOrient{0, 1, 0, m0, 0, mx};                       // S(y, x')
  if (rot == 1) return RsOrient{Hs - 1 - m0, 0, -mx, 0, 1, 0};             // S(Hs-1-x', y)
  if (rot == 2) return RsOrient{Hs - 1, -1, 0, Ws - 1 - m0, 0, -mx};       // S(Hs-1-y, Ws-1-x')
  return RsOrient{m0, 0, mx, Ws - 1, -1, 0};                               // S(x', Ws-1-y)
}

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The stored rectangle behind displayed rows [dy0, dy1] x columns [dx0, dx1], clamped into the stored frame.
__host__ __device__ __forceinline__ void rs_tile_rect(const RsOrient& o, int dy0, int dy1, int dx0, int dx1, int Hs, int Ws, int& sr0,
                                                      int& sr1, int& sc0, int& sc1) {
  const int ra = o.r0 + o.ry * dy0 + o.rx * dx0, rb = o.r0 + o.ry * dy1 + o.rx * dx1;
  const int ca = o.c0 + o.cy * dy0 + o.cx * dx0, cb = o.c0 + o.cy * dy1 + o.cx * dx1;
  sr0 = ra < rb ? ra : rb, sr1 = ra < rb ? rb : ra, sc0 = ca < cb ? ca : cb, sc1 = ca < cb ? cb : ca;
  sr0 = sr0 < 0 ? 0 : sr0, sc0 = sc0 < 0 ? 0 : sc0;
  sr1 = sr1 > Hs - 1 ? Hs - 1 : sr1, sc1 = sc1 > Ws - 1 ? Ws - 1 : sc1;
}

// The displayed rows / columns [d0, d1] the taps of outputs [first, first + n) touch.
__host__ __device__ __forceinline__ void rs_tile_range(float s, int first, int n, int n_in, int& d0, int& d1) {
  int unused;
  float lunused;
  rs_coord(s, first, n_in, d0, unused, lunused);
  rs_coord(s, first + n - 1, n_in, unused, d1, lunused);
}

// S / INTER / FORM / D / PK: as rs_strip_rgb.
template <typename S, bool INTER, int FORM, typename D, typename PK = RsDense>
__device__ __forceinline__ void rs_tile_rgb(unsigned char* lds, const RsTileLaunch& g, const RsRgbSrc& s, int orient, const RsDst& d,
                                            int zi, int t, const PK& pk = PK()) {
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int XB = PK::kPacked ? PK::PB : (INTER ? 3 : (int)sizeof(S));   // bytes from one source column to the next
  const int tid = threadIdx.x;
  const int tile_y = blockIdx.x / g.tiles_x, tile_x = blockIdx.x - tile_y * g.tiles_x;
  const int row0 = tile_y * g.TR, col0 = tile_x * g.TC;
  const int nrows = min(g.TR, d.Ho - row0), ncols = min(g.TC, d.Wo - col0);
  if (nrows <= 0 || ncols <= 0) return;
  const int planes = INTER ? 1 : d.C;
  const int pitch = g.pitch;
  const int Hd = (orient & 1) ? s.Ws : s.Hs, Wd = (orient & 1) ? s.Hs : s.Ws;
  const RsOrient o = rs_orient_map(orient, s.Hs, s.Ws);

  int dy0, dy1, dx0, dx1, sr0, sr1, sc0, sc1;
  rs_tile_range(s.sy, s.yoff + row0, nrows, Hd, dy0, dy1);
  rs_tile_range(s.sx, s.xoff + col0, ncols, Wd, dx0, dx1);
  rs_tile_rect(o, dy0, dy1, dx0, dx1, s.Hs, s.Ws, sr0, sr1, sc0, sc1);
  const int nslots = sr1 - sr0 + 1;
  const int span_bytes = (sc1 - sc0 + 1) * XB;
  if (nslots > g.rows || span_bytes + 15 > pitch) return;

  // byte address of column sc0 of stored row r of plane `pl` of the selected frame (packed: the record's pitch and stride)
  long row_bytes = (long)s.Ws * XB;
  long frame_bytes = (long)s.Hs * row_bytes;
  if constexpr (PK::kPacked) row_bytes = pk.row_bytes, frame_bytes = pk.frame_bytes;
  const long first = (s.clip_frame0 + s.ts) * frame_bytes + (long)sc0 * XB;
  const long plane_bytes = INTER ? 0 : (long)s.N * frame_bytes;
  auto row_addr = [&](int r, int pl) -> uintptr_t { return s.src + first + (long)pl * plane_bytes + (long)r * row_bytes; };

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
        const uintptr_t a = row_addr(sr0 + slot, pl);
        if (ch * 16 < (int)(a & 15) + span_bytes) {
          val[u] = *reinterpret_cast<const u32x4*>((a & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = sp * pitch + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- gather ------------------------------------------------------------------------------------------------
  float sc[4], sh[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sc[c] = (d.ch_scale && c < d.C) ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift && c < d.C) ? d.ch_shift[c] : 0.f;
  }
  // the low address bits of a staged row: 32-bit arithmetic keeps `addr & 15`
  const unsigned rb32 = (unsigned)row_bytes, pb32 = (unsigned)plane_bytes, a32 = (unsigned)(s.src + first);
  // LDS byte offset of the tap at displayed (iy, ix), plane pl (INTER: channel 0)
  auto tap = [&](int iy, int ix, int pl) -> int {
    const int r = rs_clampi(o.r0 + o.ry * iy + o.rx * ix, sr0, sr1), c = rs_clampi(o.c0 + o.cy * iy + o.cx * ix, sc0, sc1);
    const int lo = (int)((a32 + (unsigned)pl * pb32 + (unsigned)r * rb32) & 15u);
    return ((r - sr0) * planes + pl) * pitch + lo + (c - sc0) * XB;
  };
  const int gpr = (ncols + G - 1) / G;             // groups per tile row
  const int items = nrows * gpr;
  for (int it = tid; it < items; it += kRsThreads) {
    const int r = it / gpr, gx = it - r * gpr;
    const int y = row0 + r;
    int i0y, i1y;
    float ly1;
    rs_coord(s.sy, s.yoff + y, Hd, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int x0 = col0 + gx * G;
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(x0 + j, d.Wo - 1);         // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(s.sx, s.xoff + x, Wd, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      if constexpr (PK::kPacked) {                 // PB == 4: four dword reads, the channels out of the registers
        const int at[4] = {tap(i0y, i0x, 0), tap(i0y, i1x, 0), tap(i1y, i0x, 0), tap(i1y, i1x, 0)};
        unsigned w[4] = {0, 0, 0, 0};
        if constexpr (PK::PB == 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = rs_px4(lds, at[k]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float p[4];
          rs_packed_taps(pk, lds, at, w, c, p);
          out[c][j] = rs_blend_rgb(ly0, ly1, lx0, lx1, p, sc[c], sh[c]);
        }
        out[3][j] = 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < d.C) {
            const int pl = INTER ? 0 : c, cb = INTER ? c : 0;
            const float p00 = rs_tap<S>(lds, tap(i0y, i0x, pl) + cb), p01 = rs_tap<S>(lds, tap(i0y, i1x, pl) + cb);
            const float p10 = rs_tap<S>(lds, tap(i1y, i0x, pl) + cb), p11 = rs_tap<S>(lds, tap(i1y, i1x, pl) + cb);
            const float v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
            out[c][j] = v * sc[c] + sh[c];
          } else {
            out[c][j] = 0.f;
          }
        }
      }
      // packed pixels: finish this pixel before the next one starts (as in rs_strip_yuv)
      if constexpr (PK::kPacked) asm volatile("" : "+v"(out[0][j]), "+v"(out[1][j]), "+v"(out[2][j]));
    }
    const int nvalid = min(G, d.Wo - x0);
    rs_store_group<FORM, D, G>(d.dst, out, d.C, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, nvalid);
  }
}

// CSTEP / FORM / D / SMP / MAP / SUB: as rs_strip_yuv.  The shifts apply to STORED rows and columns.
// ARR: as rs_strip_yuv; the staged rectangle's rows then span the macropixels [sc0 >> 1, sc1 >> 1].
template <int CSTEP, int FORM, typename D, typename SMP, typename MAP = RsTapNone, typename SUB = RsSub420, typename ARR = RsPlanes>
__device__ __forceinline__ void rs_tile_yuv(unsigned char* lds, const RsTileLaunch& g, const RsYuvSrc& s, int orient, const RsDst& d,
                                            const float* yuv2rgb, int zi, int t, const MAP& map = MAP(), const SUB& sub = SUB()) {
  constexpr int G = RsGroup<FORM, D>::G;
  constexpr int CP = CSTEP == 1 ? 2 : 1;           // staged chroma planes
  constexpr int SB = (int)sizeof(SMP);             // bytes from one luma column to the next
  constexpr int CB = CSTEP * SB;                   // bytes from one chroma column to the next
  const int tid = threadIdx.x;
  const int tile_y = blockIdx.x / g.tiles_x, tile_x = blockIdx.x - tile_y * g.tiles_x;
  const int row0 = tile_y * g.TR, col0 = tile_x * g.TC;
  const int nrows = min(g.TR, d.Ho - row0), ncols = min(g.TC, d.Wo - col0);
  if (nrows <= 0 || ncols <= 0) return;
  const int pitch_y = g.pitch, pitch_c = g.pitch_c, c_base = g.c_base;
  const int Hd = (orient & 1) ? s.Ws : s.Hs, Wd = (orient & 1) ? s.Hs : s.Ws;
  const RsOrient o = rs_orient_map(orient, s.Hs, s.Ws);

  int dy0, dy1, dx0, dx1, sr0, sr1, sc0, sc1;
  rs_tile_range(s.sy, s.yoff + row0, nrows, Hd, dy0, dy1);
  rs_tile_range(s.sx, s.xoff + col0, ncols, Wd, dx0, dx1);
  rs_tile_rect(o, dy0, dy1, dx0, dx1, s.Hs, s.Ws, sr0, sr1, sc0, sc1);
  const int cr0 = sr0 >> sub.csy, cc0 = sc0 >> sub.csx;
  const int nslots = sr1 - sr0 + 1, ncslots = ARR::kMacro ? 0 : (sr1 >> sub.csy) - cr0 + 1;
  const int span_y = ARR::kMacro ? ((sc1 >> 1) - cc0 + 1) * CB : (sc1 - sc0 + 1) * SB;   // macropixels: one staged row, the span of both
  const int span_c = ((sc1 >> sub.csx) - cc0 + 1) * CB;
  if (nslots > g.rows || ncslots > g.rows_c || span_y + 15 > pitch_y || (!ARR::kMacro && span_c + 15 > pitch_c)) return;

  const uintptr_t frame = s.src + s.frame_off;
  // the first staged byte of stored row r: luma column sc0, or the macropixel that holds it
  auto y_addr = [&](int r) -> uintptr_t { return frame + (long)r * s.y_pitch + (ARR::kMacro ? cc0 * CB : sc0 * SB); };
  auto c_addr = [&](int cr, int pl) -> uintptr_t {
    return frame + (pl == 0 ? s.c_off_a : s.c_off_b) + (long)cr * s.c_pitch + (long)cc0 * CB;
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
        const uintptr_t a = luma ? y_addr(sr0 + slot) : c_addr(cr0 + slot, pl);
        if (ch * 16 < (int)(a & 15) + (luma ? span_y : span_c)) {
          val[u] = *reinterpret_cast<const u32x4*>((a & ~(uintptr_t)15) + (uintptr_t)ch * 16);
          off[u] = (luma ? sp * pitch_y : c_base + sp * pitch_c) + ch * 16;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4*>(lds + off[u]) = val[u];
  }
  __syncthreads();

  // ---- gather ------------------------------------------------------------------------------------------------
  float m[12], sc[3], sh[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = yuv2rgb[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sc[c] = d.ch_scale ? d.ch_scale[c] : 1.f;
    sh[c] = (d.ch_scale && d.ch_shift) ? d.ch_shift[c] : 0.f;
  }
  // the low address bits of a staged row: 32-bit arithmetic keeps `addr & 15`
  const unsigned ya32 = (unsigned)(frame + (ARR::kMacro ? cc0 * CB : sc0 * SB)), yp32 = (unsigned)s.y_pitch, cp32 = (unsigned)s.c_pitch;
  const unsigned ua32 = (unsigned)(frame + s.c_off_a + (long)cc0 * CB), va32 = (unsigned)(frame + s.c_off_b + (long)cc0 * CB);
  // LDS byte offsets of the Y, U and V samples of the tap at displayed (iy, ix)
  auto tap = [&](int iy, int ix, int& oy, int& ou, int& ov) {
    const int r = rs_clampi(o.r0 + o.ry * iy + o.rx * ix, sr0, sr1), c = rs_clampi(o.c0 + o.cy * iy + o.cx * ix, sc0, sc1);
    if constexpr (ARR::kMacro) {                   // one staged row: U, V and luma at their bytes of a macropixel
      const int row = (r - sr0) * pitch_y + (int)((ya32 + (unsigned)r * yp32) & 15u), co = ((c >> 1) - cc0) * CB;
      oy = row + rs_macro_y_byte<SB>(s.u_byte) + (c - 2 * cc0) * 2 * SB;
      ou = row + s.u_byte + co, ov = row + s.v_byte + co;
      return;
    }
    oy = (r - sr0) * pitch_y + (int)((ya32 + (unsigned)r * yp32) & 15u) + (c - sc0) * SB;
    // (RsSub420 is named by its type here: the lambda then does not capture `sub`, which changed the 4:2:0 tile kernels)
    int cr, cq;                                    // the chroma row and column of the stored pixel
    if constexpr (std::is_empty<SUB>::value) cr = r >> SUB::csy, cq = c >> SUB::csx;
    else cr = r >> sub.csy, cq = c >> sub.csx;
    const int co = (cq - cc0) * CB, crow = c_base + (cr - cr0) * CP * pitch_c;
    ou = crow + (int)((ua32 + (unsigned)cr * cp32) & 15u) + s.u_byte + co;
    ov = crow + (CP - 1) * pitch_c + (int)((va32 + (unsigned)cr * cp32) & 15u) + s.v_byte + co;
  };
  const int gpr = (ncols + G - 1) / G;             // groups per tile row
  const int items = nrows * gpr;
  for (int it = tid; it < items; it += kRsThreads) {
    const int r = it / gpr, gx = it - r * gpr;
    const int y = row0 + r;
    int i0y, i1y;
    float ly1;
    rs_coord(s.sy, s.yoff + y, Hd, i0y, i1y, ly1);
    const float ly0 = 1.f - ly1;
    const int x0 = col0 + gx * G;
    float out[4][G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int x = min(x0 + j, d.Wo - 1);         // a group cut by the right edge recomputes the last column; not stored
      int i0x, i1x;
      float lx1;
      rs_coord(s.sx, s.xoff + x, Wd, i0x, i1x, lx1);
      const float lx0 = 1.f - lx1;
      int y00, u00, v00, y10, u10, v10, y01, u01, v01, y11, u11, v11;   // (displayed row, column) of the tap
      tap(i0y, i0x, y00, u00, v00);
      tap(i1y, i0x, y10, u10, v10);
      tap(i0y, i1x, y01, u01, v01);
      tap(i1y, i1x, y11, u11, v11);
      f32x2 p0[3], p1[3];                          // {row i0y, row i1y} of column i0x / i1x, per channel
      yuv_tap2<SMP, MAP>(m, lds, y00, u00, v00, y10, u10, v10, p0, map);
      yuv_tap2<SMP, MAP>(m, lds, y01, u01, v01, y11, u11, v11, p1, map);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][j] = yuv_blend(ly0, ly1, lx0, lx1, p0[c], p1[c], sc[c], sh[c]);
      out[3][j] = 0.f;
      // finish this pixel before the next one starts (as in rs_strip_yuv)
      asm volatile("" : "+v"(out[0][j]), "+v"(out[1][j]), "+v"(out[2][j]));
    }
    rs_store_group<FORM, D, G>(d.dst, out, 3, d.T, d.Ho, d.Wo, d.c_p, d.ld, d.bs, zi, t, y, x0, min(G, d.Wo - x0));
  }
}

// ---- the item of a workgroup -------------------------------------------------------------------------------------------
// Every item-sourced kernel starts the same way: blockIdx.z loads its 16-byte item, clamps source / row / view into range
// before anything is addressed through them, loads the item's record and clamps the entry of its table row into [0, N-1] of
// that source, so a malformed item or table can never read outside the item's source.  Everything is uniform over the
// workgroup, so these are scalar loads; the record is read field by field through a pointer (a by-value copy indexed at run
// time would be scratch).  The selected frame is (src, ts): the video and the entry (whole videos), or the frame itself and 0
// (frame lists: `src` of a record is a slice of a device table of frame addresses, and the entry picks one).
// There `src` is a generic pointer loaded from memory: read through it the table entry would be a per-lane flat load.  The
// table is global memory that nothing writes while the kernel runs, so it is read as constant memory: one scalar load.
// KIND says which of the two a launch has: known at compile time (pv_batch.hip, pv_frames*.hip, whose kernels then hold no
// trace of the other kind) or asked of the workgroup-uniform kernel argument `frames`, so that one set of kernels serves both
// (pv_region.hip, pv_area.hip).  pv_orient.hip and pv_hdr.hip still carry a loader of their own that takes the same steps:
// behind this one their kernels come out with other code, and each file says what moves.
enum { RS_VIDEOS = 0, RS_FRAMES = 1, RS_EITHER = 2 };
struct RsItem {
  const pv_view_source* __restrict__ S;
  int view, orient;
  long at;              // where (row, t) lies in the frame table -- and in whatever else a launch keeps per (row, t)
  uintptr_t src;        // the video, or -- frame lists -- the selected frame
  int ts;               // the selected frame of the video, clamped; frame lists: 0
  bool list;            // `src` is a frame of a list
};
template <int KIND> __device__ __forceinline__ RsItem rs_item(const pv_batch_views_desc& d, int zi, int t, int frames = 0) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  RsItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  r.orient = r.S->orient & 7;
  const int row = min(max(it->row, 0), d.n_rows - 1);
  r.at = (long)row * d.t_stride + t;
  const int ts = min(max(d.t_index[r.at], 0), r.S->N - 1);
  r.list = KIND == RS_FRAMES || (KIND == RS_EITHER && frames);
  if (r.list) {
    typedef const uint64_t __attribute__((address_space(4))) * table_ptr;
    r.src = (uintptr_t) reinterpret_cast<table_ptr>(reinterpret_cast<uintptr_t>(r.S->src))[ts];
    r.ts = 0;
  } else {
    r.src = reinterpret_cast<uintptr_t>(r.S->src);
    r.ts = ts;
  }
  return r;
}

// The geometry a body takes, from an item's record: the stored frame, the scale, the item's window (selected, not indexed)
// and the selected frame.  Which byte of an interleaved pair is U / V, and where the staged chroma plane(s) start inside a
// frame, follow from the record's offsets.
__device__ __forceinline__ RsRgbSrc rs_item_rgb(const RsItem& item) {
  const pv_view_source* __restrict__ V = item.S;
  RsRgbSrc s;
  s.src = item.src;
  s.Hs = V->Hs, s.Ws = V->Ws, s.N = item.list ? 1 : V->N;   // a frame of a list is dense [C, Hs, Ws]: the plane stride of ONE frame
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.ts = item.ts;
  s.clip_frame0 = 0;
  return s;
}
template <int CSTEP> __device__ __forceinline__ RsYuvSrc rs_item_yuv(const RsItem& item) {
  const pv_view_source* __restrict__ V = item.S;
  RsYuvSrc s;
  s.src = item.src;
  s.frame_off = (long)item.ts * V->frame_stride;
  s.Hs = V->Hs, s.Ws = V->Ws;
  s.sy = V->sy, s.sx = V->sx;
  s.yoff = rs_view_off(item.view, V->y_off[0], V->y_off[1], V->y_off[2]);
  s.xoff = rs_view_off(item.view, V->x_off[0], V->x_off[1], V->x_off[2]);
  s.y_pitch = V->y_pitch, s.c_pitch = V->c_pitch;
  rs_chroma_planes(CSTEP == 2, V->u_offset, V->v_offset, s);
  return s;
}

// The shared item with what is pv_region_views' own on top (pv_region.hip, and its packed kernels in pv_packed.hip): the
// rectangle of the item's (row, t), clamped into the stored frame before any address is formed -- top / left inside it, h / w
// at least 1 and ending inside it -- and its sy / sx.
// (One function, the loader's call inside it: with the rectangle read by a function of its own behind the loader, its loads
// are ordered otherwise and every kernel of pv_region.hip changes -- profiles/r24/isa_vs_parent.md.)
struct RgItem : RsItem {
  int top, left, h, w;
  float sy, sx;
};
__device__ __forceinline__ RgItem rg_item(const pv_batch_views_desc& d, const pv_view_region* __restrict__ regions, int frames, int zi,
                                          int t) {
  RgItem r{rs_item<RS_EITHER>(d, zi, t, frames)};
  const pv_view_region* __restrict__ G = regions + r.at;
  const int Hs = r.S->Hs, Ws = r.S->Ws;
  r.top = min(max(G->top, 0), Hs - 1), r.left = min(max(G->left, 0), Ws - 1);
  r.h = min(max(G->h, 1), Hs - r.top), r.w = min(max(G->w, 1), Ws - r.left);
  r.sy = G->sy, r.sx = G->sx;
  return r;
}
// The geometry of rs_strip_rgb over that rectangle: the stored frame keeps the strides, the body's source is the rectangle.
__device__ __forceinline__ RsRgbWin rg_item_rgb(const RgItem& item) {
  RsRgbWin s;
  static_cast<RsRgbSrc&>(s) = rs_item_rgb(item);
  s.Hf = s.Hs, s.Wf = s.Ws;
  s.top = item.top, s.left = item.left;
  s.Hs = item.h, s.Ws = item.w;
  s.sy = item.sy, s.sx = item.sx;
  s.yoff = 0, s.xoff = 0;
  return s;
}

// ---- the launch arithmetic shared by the entry points ---------------------------------------------------------------
// Folds the widest source column span of a record's views into `span`, and the chroma span behind it into `span_c`, both in
// columns: times the bytes of a column (rs_yuv_pitches for YUV) they size the staged rows.
// csx: the chroma column shift of the launch (rs_yuv_sub; ignored by the RGB / planar forms, which do not read span_c).
inline void rs_widest_span(float sx, const int32_t* x_off, int n_views, int Wo, int Ws, int& span, int& span_c, int csx = 1) {
  for (int v = 0; v < n_views; ++v) {
    int a, b, u;
    float l;
    rs_coord(sx, x_off[v], Ws, a, u, l);
    rs_coord(sx, x_off[v] + Wo - 1, Ws, u, b, l);
    span = b - a + 1 > span ? b - a + 1 : span;
    const int c = (b >> csx) - (a >> csx) + 1;
    span_c = c > span_c ? c : span_c;
  }
}

// The LDS pitches of a staged luma row and a staged chroma (row, plane) for the widest spans (columns) of a launch whose
// samples have `sb` bytes, and the LDS bytes of the two source rows of one output row with their chroma.  c_step 4 is the
// macropixel arrangement (RsMacro), whose widest macropixel span is span_c.
inline long rs_yuv_pitches(int span, int span_c, int c_step, int sb, int32_t& pitch_y, int32_t& pitch_c) {
  if (c_step == 4) {                               // packed 4:2:2: one staged row of span_c macropixels, no chroma image
    pitch_y = pv_round_up(span_c * 4 * sb + 15, 16), pitch_c = 0;
    return 2L * pitch_y;
  }
  pitch_y = pv_round_up(span * sb + 15, 16);
  pitch_c = pv_round_up(span_c * c_step * sb + 15, 16);
  return 2L * (pitch_y + (long)(c_step == 2 ? 1 : 2) * pitch_c);
}

// R output rows per workgroup and the LDS bytes they stage; per_row: LDS bytes of the two source rows of one output row.
inline int rs_strip_rows(long per_row, int Ho, int32_t& R_out, size_t& lds) {
  long R = kRsLdsBudget / per_row;
  R = R > kRsMaxRows ? kRsMaxRows : R;
  R = R > Ho ? Ho : R;
  if (R < 1) R = 1;
  if (R * per_row > kRsLdsMax) return PV_ERR_UNSUPPORTED;
  R_out = (int32_t)R;
  lds = (size_t)(R * per_row);
  return PV_OK;
}

// The LDS pitch of a staged RGB / planar (row, plane) for the widest span (columns) of a launch.
inline int32_t rs_rgb_pitch(int span, int src_layout, int src_dtype) {
  const int pb = rs_packed_px(src_layout);         // packed pixels: PB bytes per column
  return pv_round_up(span * (pb ? pb : (src_layout == PV_SRC_NTHWC ? 3 : (src_dtype == PV_F32 ? 4 : 1))) + 15, 16);
}
// Frame-interleaved sources stage ONE plane per row: [.., 3] and the packed layouts.
inline bool rs_interleaved(int src_layout) { return src_layout == PV_SRC_NTHWC || rs_packed_px(src_layout) != 0; }

// The LDS layout of a staged tile (RsTileLaunch, or a launch struct with the same fields: pv_area.hip) whose widest footprint
// is n = {rows, columns, chroma rows, chroma columns}: every staged row of every plane at its pitch, for YUV the chroma image
// behind the luma one.  Returns the bytes, not yet narrowed to 32 bits.
template <typename Launch> inline long rs_tile_layout(const pv_batch_views_desc& d, const int (&n)[4], Launch& g) {
  g.rows = n[0], g.rows_c = n[2];
  if (rs_yuv_sub(d.src_layout)) {
    rs_yuv_pitches(n[1], n[3], d.c_step, d.src_dtype == PV_U16 ? 2 : 1, g.pitch, g.pitch_c);
    g.c_base = g.rows * g.pitch;
    return (long)g.c_base + (long)g.rows_c * (d.c_step == 2 ? 1 : 2) * g.pitch_c;   // packed 4:2:2: pitch_c is 0
  }
  g.pitch = rs_rgb_pitch(n[1], d.src_layout, d.src_dtype);
  return (long)g.rows * (rs_interleaved(d.src_layout) ? 1 : d.C) * g.pitch;
}

// The destination-form dispatch: KERNEL<leading template arguments..., FORM, D>ARGS over a grid of GRID_X workgroups (strips,
// or tiles) x d.T frames x d.n_items destination items with LDS bytes of staging.  ARGS is the kernel's argument list in
// parentheses; expects d (the descriptor the destination is read from) and stream in scope.
#define RS_ARGS(...) __VA_ARGS__
#define RS_DISPATCH(GRID_X, LDS, ARGS, KERNEL, ...)                                                                      \
  do {                                                                                                                   \
    const dim3 grid((unsigned)(GRID_X), (unsigned)d.T, (unsigned)d.n_items), block(kRsThreads);                          \
    hipStream_t s = static_cast<hipStream_t>(stream);                                                                    \
    if (d.dst_layout == PV_DST_NCTHW) {                                                                                  \
      if (d.dst_dtype == PV_BF16) PV_LAUNCH((KERNEL<__VA_ARGS__, RS_PLANAR, bf16_t>), grid, block, LDS, s, RS_ARGS ARGS); \
      else PV_LAUNCH((KERNEL<__VA_ARGS__, RS_PLANAR, float>), grid, block, LDS, s, RS_ARGS ARGS);                        \
    } else if (d.c_p == 4) {                                                                                             \
      PV_LAUNCH((KERNEL<__VA_ARGS__, RS_C4, bf16_t>), grid, block, LDS, s, RS_ARGS ARGS);                                \
    } else {                                                                                                             \
      if (d.dst_dtype == PV_BF16) PV_LAUNCH((KERNEL<__VA_ARGS__, RS_CL, bf16_t>), grid, block, LDS, s, RS_ARGS ARGS);    \
      else PV_LAUNCH((KERNEL<__VA_ARGS__, RS_CL, float>), grid, block, LDS, s, RS_ARGS ARGS);                            \
    }                                                                                                                    \
  } while (0)

// The source-form dispatch of an item-sourced launch in front of it: YUV(CSTEP, SMP) for YUV 4:2:0 -- two-byte or one-byte
// samples, one interleaved chroma plane or two -- else RGB(S, INTER) for [T, H, W, 3] bytes and for planar bytes / fp32.
// RGB and YUV are the unit's own macros, as a rule one RS_DISPATCH each; expects d in scope.
#define RS_SOURCE_FORMS(RGB, YUV)                                                                                        \
  do {                                                                                                                   \
    if (d.src_layout == PV_SRC_YUV420 && d.src_dtype == PV_U16) {                                                        \
      if (d.c_step == 2) YUV(2, unsigned short);                                                                         \
      else YUV(1, unsigned short);                                                                                       \
    } else if (d.src_layout == PV_SRC_YUV420) {                                                                          \
      if (d.c_step == 2) YUV(2, unsigned char);                                                                          \
      else YUV(1, unsigned char);                                                                                        \
    } else if (d.src_layout == PV_SRC_NTHWC) {                                                                           \
      RGB(unsigned char, true);                                                                                          \
    } else if (d.src_dtype == PV_U8) {                                                                                   \
      RGB(unsigned char, false);                                                                                         \
    } else {                                                                                                             \
      RGB(float, false);                                                                                                 \
    }                                                                                                                    \
  } while (0)

// ---- host-side checks shared by the entry points ------------------------------------------------------------------
// The crop windows of every view lie inside the scaled frame.
inline int rs_check_views(int n_views, const int32_t* y_off, const int32_t* x_off, int Ho, int Wo, int Hn, int Wn) {
  if (n_views < 1 || n_views > 3) return PV_ERR_INVALID;
  for (int v = 0; v < n_views; ++v)
    if (y_off[v] < 0 || x_off[v] < 0 || (long)y_off[v] + Ho > Hn || (long)x_off[v] + Wo > Wn) return PV_ERR_INVALID;
  return PV_OK;
}

// Items [item0, item0 + n_items) of a sequence of all_items (n_items == 0 with item0 == 0: all of it), within the grid.
inline int rs_check_items(int32_t item0, int32_t& n_items, long all_items, int T) {
  if (n_items == 0 && item0 == 0) n_items = (int32_t)all_items;
  if (item0 < 0 || n_items <= 0 || (long)item0 + n_items > all_items) return PV_ERR_INVALID;
  if (T > 65535 || n_items > 65535) return PV_ERR_INVALID;   // grid.y / grid.z
  return PV_OK;
}

// The destination matrix: dtype / layout pairs and their alignment.
inline int rs_check_dst(const void* dstp, int dst_layout, int dst_dtype, int c_p, int ld, int64_t bs, int T, int Ho, int Wo) {
  if (dst_dtype != PV_BF16 && dst_dtype != PV_F32) return PV_ERR_UNSUPPORTED;
  const uintptr_t dst = reinterpret_cast<uintptr_t>(dstp);
  if (dst_layout == PV_DST_NDHWC) {
    if (c_p == 4 && ld == 4) {
      if (dst_dtype != PV_BF16) return PV_ERR_UNSUPPORTED;
      if (bs % 4 || dst % 8) return PV_ERR_INVALID;
    } else if (c_p >= 8 && c_p % 8 == 0) {
      if (ld % 8 || ld < c_p || bs % 8 || dst % 16) return PV_ERR_INVALID;
    } else {
      return PV_ERR_UNSUPPORTED;
    }
    if (bs < (int64_t)T * Ho * Wo * ld) return PV_ERR_INVALID;
  } else if (dst_layout == PV_DST_NCTHW) {
    if (dst % (dst_dtype == PV_BF16 ? 2 : 4)) return PV_ERR_INVALID;
  } else {
    return PV_ERR_UNSUPPORTED;
  }
  return PV_OK;
}

// Bytes [off, off + (rows - 1) * pitch + (cols - 1) * step + sb) of a plane of sb-byte samples lie inside [0, frame_stride).
inline bool plane_inside(int64_t off, int64_t rows, int64_t pitch, int64_t cols, int64_t step, int64_t frame_stride, int64_t sb = 1) {
  return off >= 0 && off + (rows - 1) * pitch + (cols - 1) * step + (sb - 1) < frame_stride;
}

// The planes of one YUV frame of Hs x Ws (both positive) of sb-byte samples: a size the subsampling halves is even (4:2:0: both;
// 4:2:2: Ws; 4:4:4: neither), the chroma form (c_step counts samples), pitches that hold a row, and luma and chroma planes --
// Hs >> csy rows of Ws >> csx samples -- inside [0, frame_stride).  Pitches, offsets and the frame stride are bytes.
// c_step 4 is the ONE plane of packed 4:2:2 (the caller has matched it with the layout: rs_check_item_desc): rows of Ws / 2
// macropixels of four samples at y_pitch, no chroma pitch, and u_offset / v_offset the bytes of U / V inside a macropixel --
// two different samples of it that are both even or both odd, which leaves luma the other two.
inline int rs_check_yuv_planes(int Hs, int Ws, int c_step, int y_pitch, int c_pitch, int64_t frame_stride, int64_t u_offset,
                               int64_t v_offset, int sb = 1, RsSub c = RsSub{1, 1}) {
  if (((c.csy ? Hs : 0) | (c.csx ? Ws : 0)) & 1) return PV_ERR_INVALID;
  if (c_step == 4) {
    if (c.csy != 0 || c.csx != 1 || c_pitch != 0) return PV_ERR_INVALID;
    const int64_t row = 2 * (int64_t)Ws * sb;
    if (y_pitch < row || frame_stride < (int64_t)(Hs - 1) * y_pitch + row) return PV_ERR_INVALID;
    const int64_t du = u_offset - v_offset;
    if (u_offset < 0 || v_offset < 0 || u_offset >= 4 * sb || v_offset >= 4 * sb || u_offset % sb || (du != 2 * sb && du != -2 * sb))
      return PV_ERR_INVALID;
    return PV_OK;
  }
  if (c_step != 1 && c_step != 2) return PV_ERR_INVALID;
  const int Hc = Hs >> c.csy, Wc = Ws >> c.csx;
  if (y_pitch < (int64_t)Ws * sb || c_pitch < (int64_t)Wc * c_step * sb || frame_stride <= 0) return PV_ERR_INVALID;
  if (c_step == 2 && v_offset - u_offset != sb && u_offset - v_offset != sb) return PV_ERR_INVALID;
  if (!plane_inside(0, Hs, y_pitch, Ws, sb, frame_stride, sb) ||
      !plane_inside(u_offset, Hc, c_pitch, Wc, (int64_t)c_step * sb, frame_stride, sb) ||
      !plane_inside(v_offset, Hc, c_pitch, Wc, (int64_t)c_step * sb, frame_stride, sb))
    return PV_ERR_INVALID;
  return PV_OK;
}

// Two-byte samples: every sample address is even, so that the 16-bit LDS reads of the gather are naturally aligned (the LDS
// image of a staged row keeps the row's `addr & 15`).  `base` is the source or, for a frame list, a frame's address.
inline bool rs_yuv16_even(uintptr_t base) { return (base & 1) == 0; }
inline int rs_check_yuv16_even(uintptr_t base, int y_pitch, int c_pitch, int64_t frame_stride, int64_t u_offset, int64_t v_offset) {
  if (!rs_yuv16_even(base) || ((y_pitch | c_pitch) & 1) || ((frame_stride | u_offset | v_offset) & 1)) return PV_ERR_INVALID;
  return PV_OK;
}

// ---- an item-sourced launch (pv_batch_views, pv_frame_views): validated and sized here, once -----------------------------
inline bool rs_same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// check_src of a launch whose records are whole videos (pv_batch_views; pv_hdr_views without a pointer table): `src` is one
// allocation of the source dtype, 4-byte aligned for fp32, even for 16-bit samples.
inline auto rs_check_video_src(int src_dtype, int src_layout = PV_SRC_NCTHW) {
  // address bits `src` may not have (4-byte pixels: a pixel is one aligned dword)
  const uintptr_t misaligned = src_dtype == PV_F32 || rs_packed_px(src_layout) == 4 ? 3 : (src_dtype == PV_U16 ? 1 : 0);
  return [=](const pv_view_source& v) { return reinterpret_cast<uintptr_t>(v.src) & misaligned ? PV_ERR_INVALID : PV_OK; };
}

// The part of a record's check that does not depend on the views (all that pv_region_views checks of a record: its geometry is
// per frame): the stored frames -- positive sizes, the orientation code, for YUV the planes -- and what `src` points to.
template <typename CheckSrc>
inline int rs_check_record_frames(const pv_batch_views_desc& d, const pv_view_source& v, bool yuv, const CheckSrc& check_src) {
  if (!v.src || v.N <= 0 || v.Hs <= 0 || v.Ws <= 0) return PV_ERR_INVALID;
  if (v.orient < 0 || v.orient > 7) return PV_ERR_INVALID;
  if (yuv) {
    const int sb = d.src_dtype == PV_U16 ? 2 : 1;
    RsSub c = {1, 1};
    rs_yuv_sub(d.src_layout, &c);
    if (int e = rs_check_yuv_planes(v.Hs, v.Ws, d.c_step, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset, sb, c)) return e;
    if (sb == 2 && rs_check_yuv16_even(0, v.y_pitch, v.c_pitch, v.frame_stride, v.u_offset, v.v_offset)) return PV_ERR_INVALID;
  }
  if (const int pb = rs_packed_px(d.src_layout)) {   // packed pixels: a pitch that holds a row, a stride that holds a frame, dwords aligned
    if (v.y_pitch < (int64_t)v.Ws * pb || v.frame_stride < (int64_t)(v.Hs - 1) * v.y_pitch + (int64_t)v.Ws * pb) return PV_ERR_INVALID;
    if (v.u_offset != 0 || v.v_offset != 0 || v.c_pitch != 0) return PV_ERR_INVALID;
    if (pb == 4 && ((v.y_pitch | v.frame_stride) & 3)) return PV_ERR_INVALID;
  }
  return check_src(v);
}

// One record of such a launch: positive sizes, windows inside the scaled frame, sy / sx the library's own division, for YUV
// the planes inside a frame, at even bytes for two-byte samples, and what its `src` points to (check_src: see below).
template <typename CheckSrc>
inline int rs_check_record(const pv_batch_views_desc& d, const pv_view_source& v, bool yuv, const CheckSrc& check_src) {
  if (v.Hn <= 0 || v.Wn <= 0) return PV_ERR_INVALID;
  if (int e = rs_check_record_frames(d, v, yuv, check_src)) return e;
  if (int e = rs_check_views(d.n_views, v.y_off, v.x_off, d.Ho, d.Wo, v.Hn, v.Wn)) return e;
  const int Hd = (v.orient & 1) ? v.Ws : v.Hs, Wd = (v.orient & 1) ? v.Hs : v.Ws;   // the displayed frame: Hn, Wn and the windows are its
  if (!rs_same_bits(v.sy, (float)Hd / (float)v.Hn) || !rs_same_bits(v.sx, (float)Wd / (float)v.Wn)) return PV_ERR_INVALID;
  return PV_OK;
}

// The widest stored footprint of a TR x TC tile of oriented record v over its views: stored rows x columns, and the chroma
// rows x columns behind them.  The map takes displayed rows to one stored axis and displayed columns to the other, so the
// bands of tile rows and of tile columns are walked separately, with the very calls the kernel makes.
inline void rs_tile_footprint(const pv_view_source& v, int n_views, int Ho, int Wo, int TR, int TC, int (&n)[4],
                              RsSub sub = RsSub{1, 1}) {
  const bool turned = v.orient & 1;
  const int Hd = turned ? v.Ws : v.Hs, Wd = turned ? v.Hs : v.Ws;
  const RsOrient o = rs_orient_map(v.orient, v.Hs, v.Ws);
  auto fold = [&](int lo, int hi, bool rows) {     // a stored interval of rows / of columns
    const int cs = rows ? sub.csy : sub.csx;
    const int a = hi - lo + 1, c = (hi >> cs) - (lo >> cs) + 1;
    int& na = n[rows ? 0 : 1];
    int& nc = n[rows ? 2 : 3];
    na = a > na ? a : na, nc = c > nc ? c : nc;
  };
  for (int view = 0; view < n_views; ++view) {
    int d0, d1, sr0, sr1, sc0, sc1;
    for (int row0 = 0; row0 < Ho; row0 += TR) {
      rs_tile_range(v.sy, v.y_off[view] + row0, TR < Ho - row0 ? TR : Ho - row0, Hd, d0, d1);
      rs_tile_rect(o, d0, d1, 0, 0, v.Hs, v.Ws, sr0, sr1, sc0, sc1);
      turned ? fold(sc0, sc1, false) : fold(sr0, sr1, true);
    }
    for (int col0 = 0; col0 < Wo; col0 += TC) {
      rs_tile_range(v.sx, v.x_off[view] + col0, TC < Wo - col0 ? TC : Wo - col0, Wd, d0, d1);
      rs_tile_rect(o, 0, 0, d0, d1, v.Hs, v.Ws, sr0, sr1, sc0, sc1);
      turned ? fold(sr0, sr1, true) : fold(sc0, sc1, false);
    }
  }
}

// TR x TC, the staged rows and the LDS pitch(es) of a tile launch over `records` (the oriented records the launch's items
// name): the largest tile of the list whose widest footprint fits the staging budget, else the smallest one if it fits the
// LDS limit.  Tiles are square-ish so that the staged rows of a transposing record stay several 16-byte granules long.
inline int rs_tile_size(const pv_batch_views_desc& d, const pv_view_source* const* records, size_t n_records, RsTileLaunch& g,
                        size_t& lds) {
  static const int tiles[][2] = {{32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {2, 8}, {1, 8}};
  for (size_t k = 0; k < sizeof(tiles) / sizeof(tiles[0]); ++k) {
    const int TR = tiles[k][0], TC = tiles[k][1];
    int n[4] = {0, 0, 0, 0};
    RsSub sub = {1, 1};
    rs_yuv_sub(d.src_layout, &sub);
    for (size_t i = 0; i < n_records; ++i) rs_tile_footprint(*records[i], d.n_views, d.Ho, d.Wo, TR, TC, n, sub);
    g = {};
    g.TR = TR, g.TC = TC, g.tiles_x = (int32_t)pv_ceil_div(d.Wo, TC);
    const long bytes = rs_tile_layout(d, n, g);
    lds = (size_t)bytes;
    if (bytes <= kRsLdsBudget) return PV_OK;
    if (k + 1 == sizeof(tiles) / sizeof(tiles[0])) return bytes <= kRsLdsMax ? PV_OK : PV_ERR_UNSUPPORTED;
  }
  return PV_ERR_UNSUPPORTED;
}

// The launch fields of an item-sourced descriptor: pointers, counts, the source form and the destination.
inline int rs_check_item_desc(const pv_batch_views_desc& d) {
  if (!d.sources || !d.sources_dev || !d.items || !d.items_dev || !d.t_index || !d.dst) return PV_ERR_INVALID;
  if (d.n_sources <= 0 || d.n_items <= 0 || d.n_rows <= 0 || d.T <= 0 || d.C <= 0 || d.Ho <= 0 || d.Wo <= 0) return PV_ERR_INVALID;
  if (d.t_stride < d.T || d.n_items > 65535 || d.T > 65535) return PV_ERR_INVALID;   // grid.y / grid.z
  if (d.C > 4 || d.n_views < 1 || d.n_views > 3) return PV_ERR_INVALID;
  const bool yuv = rs_yuv_sub(d.src_layout), inter = rs_interleaved(d.src_layout);   // [.., 3] or packed pixels
  if (!yuv && !inter && d.src_layout != PV_SRC_NCTHW) return PV_ERR_INVALID;
  if (!yuv && d.src_dtype == PV_U16) return PV_ERR_UNSUPPORTED;   // 16-bit samples are a YUV source only
  if (inter && (d.src_dtype != PV_U8 || d.C != 3)) return PV_ERR_INVALID;
  if (yuv && (!d.yuv2rgb || d.C != 3 || (rs_yuyv(d.src_layout) ? d.c_step != 4 : (d.c_step != 1 && d.c_step != 2)))) return PV_ERR_INVALID;
  // the dtype / layout matrix
  if (yuv ? (d.src_dtype != PV_U8 && d.src_dtype != PV_U16) : (d.src_dtype != PV_U8 && d.src_dtype != PV_F32)) return PV_ERR_UNSUPPORTED;
  return rs_check_dst(d.dst, d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs, d.T, d.Ho, d.Wo);
}

// R, the LDS pitch(es) and the LDS bytes of a strip launch whose widest column span is `span` (chroma: `span_c`).
inline int rs_strip_size(const pv_batch_views_desc& d, int span, int span_c, RsItemLaunch& g, size_t& lds) {
  long per_row;                                    // LDS bytes of the two source rows of one output row
  if (rs_yuv_sub(d.src_layout)) {
    per_row = rs_yuv_pitches(span, span_c, d.c_step, d.src_dtype == PV_U16 ? 2 : 1, g.pitch, g.pitch_c);
  } else {
    g.pitch = rs_rgb_pitch(span, d.src_layout, d.src_dtype);
    per_row = 2L * (rs_interleaved(d.src_layout) ? 1 : d.C) * g.pitch;
  }
  if (int e = rs_strip_rows(per_row, d.Ho, g.R, lds)) return e;
  g.c_base = 2 * g.R * g.pitch;
  return PV_OK;
}

// The walk over the items of a launch, in order: the range of source / row / view, then check(record) -- rs_check_record or
// rs_check_record_frames with the entry point's check_src -- then each(item, record, again), which sizes the launch from the
// record and may refuse the item (what a launch keeps per row: pv_region.hip).  The first refusal ends the walk and is
// returned.  A launch is a window of a longer sequence and reads only the records its items name (the kernel clamps `source`
// into range and the items are the validated ones), so its cost does not grow with the number of videos of the whole
// sequence; a video-major sequence names the record just checked (`again`), which is not checked again, and any other record
// named again is, which is cheaper than remembering.
template <typename Check, typename Each>
inline int rs_walk_items(const pv_batch_views_desc& d, const Check& check, const Each& each) {
  for (int i = 0; i < d.n_items; ++i) {
    const pv_view_item& it = d.items[i];
    if (it.source < 0 || it.source >= d.n_sources || it.row < 0 || it.row >= d.n_rows || it.view < 0 || it.view >= d.n_views)
      return PV_ERR_INVALID;
    const pv_view_source& v = d.sources[it.source];
    const bool again = i > 0 && it.source == d.items[i - 1].source;
    if (!again)
      if (int e = check(v)) return e;
    if (int e = each(it, v, again)) return e;
  }
  return PV_OK;
}

// The descriptor, the items and the record behind each of them, then the sizes of the launch.  check_src(record) is the
// entry point's own part: whether the record's `src` is a source of d.src_dtype (PV_ERR_INVALID if not).  Items of upright
// records (orient == 0) run the staged strip, sized by the widest column span(s) of any such record x view: g / lds
// (g.R == 0: the launch has none).  Items of oriented records run the staged tile: tg / lds_t (tg.TR == 0: none).
template <typename CheckSrc>
inline int rs_item_launch(const pv_batch_views_desc& d, const CheckSrc& check_src, RsItemLaunch& g, size_t& lds, RsTileLaunch& tg,
                          size_t& lds_t) {
  if (int e = rs_check_item_desc(d)) return e;
  RsSub sub = {1, 1};
  const bool yuv = rs_yuv_sub(d.src_layout, &sub);
  int span = 0, span_c = 0, n_upright = 0;
  std::vector<const pv_view_source*> oriented;     // the oriented records the items name, a video-major run once
  const auto check = [&](const pv_view_source& v) { return rs_check_record(d, v, yuv, check_src); };
  const auto each = [&](const pv_view_item&, const pv_view_source& v, bool again) {
    if (v.orient != 0) {
      if (!again) oriented.push_back(&v);
    } else {
      ++n_upright;
      rs_widest_span(v.sx, v.x_off, d.n_views, d.Wo, v.Ws, span, span_c, sub.csx);
    }
    return PV_OK;
  };
  if (int e = rs_walk_items(d, check, each)) return e;
  g = {}, tg = {};
  lds = lds_t = 0;
  if (!oriented.empty())
    if (int e = rs_tile_size(d, oriented.data(), oriented.size(), tg, lds_t)) return e;
  if (n_upright == 0) return PV_OK;
  return rs_strip_size(d, span, span_c, g, lds);
}

// The launches of a validated item sequence: every maximal run of items of one kind -- upright records, oriented records --
// is one call of `upright` / `oriented` with a descriptor whose items, item count and destination are the run's (item i of a
// launch is written to position i of dst).  A launch of upright records only is one call with the descriptor itself.
template <typename Upright, typename Oriented>
inline int rs_item_runs(const pv_batch_views_desc& d, const Upright& upright, const Oriented& oriented) {
  const long item_bytes = (d.dst_dtype == PV_BF16 ? 2L : 4L) * (d.dst_layout == PV_DST_NCTHW ? (long)d.C * d.T * d.Ho * d.Wo : (long)d.bs);
  for (int i = 0; i < d.n_items;) {
    const bool turned = d.sources[d.items[i].source].orient != 0;
    int j = i + 1;
    while (j < d.n_items && (d.sources[d.items[j].source].orient != 0) == turned) ++j;
    pv_batch_views_desc r = d;
    r.items += i, r.items_dev += i, r.n_items = j - i;
    r.dst = static_cast<unsigned char*>(d.dst) + (long)i * item_bytes;
    if (int e = turned ? oriented(r) : upright(r)) return e;
    i = j;
  }
  return PV_OK;
}

}  // namespace
