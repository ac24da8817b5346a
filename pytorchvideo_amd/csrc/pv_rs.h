// What the resampling ingest kernels share (pv_resample.hip: RGB / planar sources; pv_yuv.hip: YUV 4:2:0 sources;
// pv_batch.hip: either, with one source per destination item): the pinned source coordinate, the taps of a staged row, the
// YUV tap conversion and blend, the destination forms with their stores, and the host-side checks of views, item range,
// destination and YUV planes.  Everything is inline in an anonymous namespace: each translation unit keeps its own kernels.
#pragma once
#include "pv_common.h"

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

// ---- taps and blends shared by the one-source kernels and the per-item kernels (pv_batch.hip) ------------------------
// One tap of a staged RGB / planar row, in the source dtype.
template <typename S> __device__ __forceinline__ float rs_tap(const unsigned char* lds, int off);
template <> __device__ __forceinline__ float rs_tap<unsigned char>(const unsigned char* lds, int off) { return (float)lds[off]; }
template <> __device__ __forceinline__ float rs_tap<float>(const unsigned char* lds, int off) {
  return *reinterpret_cast<const float*>(lds + off);
}

__device__ __forceinline__ f32x2 yuv_splat(float v) { return f32x2{v, v}; }

// Two taps of the virtual RGB frame -- the same column of the two source rows -- as packed fp32 pairs (v_pk_fma_f32 does
// both for the price of one): per channel three fused multiply-adds in the header's order, then the clamp.
__device__ __forceinline__ void yuv_tap2(const float (&m)[12], const unsigned char* lds, int oy0, int ou0, int ov0, int oy1, int ou1,
                                         int ov1, f32x2 (&rgb)[3]) {
  const f32x2 Y = {(float)lds[oy0], (float)lds[oy1]}, U = {(float)lds[ou0], (float)lds[ou1]}, V = {(float)lds[ov0], (float)lds[ov1]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const f32x2 v = __builtin_elementwise_fma(yuv_splat(m[c * 4 + 2]), V, __builtin_elementwise_fma(yuv_splat(m[c * 4 + 1]), U,
                        __builtin_elementwise_fma(yuv_splat(m[c * 4]), Y, yuv_splat(m[c * 4 + 3]))));
    rgb[c] = f32x2{fminf(fmaxf(v[0], 0.f), 255.f), fminf(fmaxf(v[1], 0.f), 255.f)};
  }
}

// The pinned blend and the affine map with the contraction spelled out, so that every instantiation gives the same bits:
// p0 / p1 hold column i0x / i1x of the rows (i0y, i1y); h = {top, bottom} = lx1 p1 + (lx0 p0), v = ly1 bottom + (ly0 top).
__device__ __forceinline__ float yuv_blend(float ly0, float ly1, float lx0, float lx1, f32x2 p0, f32x2 p1, float sc, float sh) {
#pragma clang fp contract(off)
  const f32x2 h = __builtin_elementwise_fma(yuv_splat(lx1), p1, yuv_splat(lx0) * p0);
  const float v = fmaf(ly1, h[1], ly0 * h[0]);
  return fmaf(v, sc, sh);
}

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

// Bytes [off, off + (rows - 1) * pitch + (cols - 1) * step] of a plane lie inside [0, frame_stride).
inline bool plane_inside(int64_t off, int64_t rows, int64_t pitch, int64_t cols, int64_t step, int64_t frame_stride) {
  return off >= 0 && off + (rows - 1) * pitch + (cols - 1) * step < frame_stride;
}

// The planes of one YUV 4:2:0 frame of Hs x Ws (both positive): even sizes, the chroma form, pitches that hold a row, and
// luma and chroma planes inside [0, frame_stride).
inline int rs_check_yuv_planes(int Hs, int Ws, int c_step, int y_pitch, int c_pitch, int64_t frame_stride, int64_t u_offset,
                               int64_t v_offset) {
  if ((Hs | Ws) & 1) return PV_ERR_INVALID;
  if (c_step != 1 && c_step != 2) return PV_ERR_INVALID;
  if (y_pitch < Ws || c_pitch < (Ws / 2) * c_step || frame_stride <= 0) return PV_ERR_INVALID;
  if (c_step == 2 && v_offset - u_offset != 1 && u_offset - v_offset != 1) return PV_ERR_INVALID;
  if (!plane_inside(0, Hs, y_pitch, Ws, 1, frame_stride) || !plane_inside(u_offset, Hs / 2, c_pitch, Ws / 2, c_step, frame_stride) ||
      !plane_inside(v_offset, Hs / 2, c_pitch, Ws / 2, c_step, frame_stride))
    return PV_ERR_INVALID;
  return PV_OK;
}

}  // namespace
