// Layout changes at the ends of the forward path: the caller's contiguous NCDHW clip -> padded NDHWC rows (ingest: with a
// frame table and a per-channel scale / shift) and back (egress).  8-channel chunks (16 B of bf16) per thread.
#include "pv_common.h"

namespace {

constexpr int kThreads = 256;

template <typename S> __device__ __forceinline__ float ld_as_f32(const S* p) { return (float)*p; }

// ---- the stages every ingest kernel has ----
// Where destination voxel sp (of T*H*W) of a clip is read: frame t of the destination is frame t_index[t] of a source clip of
// src_T frames.  S3s: voxels of one source channel; sps: the voxel's offset inside it.
struct IngestSrc { long S3s, sps; };
__device__ __forceinline__ IngestSrc ingest_src(const pv_layout_desc& d, long sp) {
  const long HW = (long)d.H * d.W;
  const int t = (int)(sp / HW);
  IngestSrc o;
  o.S3s = (long)(d.t_index ? d.src_T : d.T) * HW;
  o.sps = (long)(d.t_index ? d.t_index[t] : t) * HW + (sp - (long)t * HW);
  return o;
}
// the per-channel scale / shift of a descriptor that has a ch_scale: v * a + c
struct ChAffine {
  float a, c;
  __device__ __forceinline__ float operator()(float v) const { return v * a + c; }
};
__device__ __forceinline__ ChAffine ingest_affine(const pv_layout_desc& d, int ch) {
  return ChAffine{d.ch_scale[ch], d.ch_shift ? d.ch_shift[ch] : 0.f};
}

// NCDHW (contiguous) -> NDHWC padded.  Thread = (voxel fastest, chunk).
template <typename S, typename T>
__global__ __launch_bounds__(kThreads) void ingest_kernel(const pv_layout_desc d, long nvox) {
  const int CG = d.c_p / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= nvox * CG) return;
  const long vox = id % nvox;
  const int cg = (int)(id / nvox);
  const long S3 = (long)d.T * d.H * d.W;
  const int b = (int)(vox / S3);
  const long sp = vox - (long)b * S3;
  const IngestSrc at = ingest_src(d, sp);
  const S* src = static_cast<const S*>(d.src) + (long)b * d.C * at.S3s + at.sps;
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cg * 8 + j;
    float v = c < d.C ? ld_as_f32(src + (long)c * at.S3s) : 0.f;
    if (c < d.C && d.ch_scale) v = ingest_affine(d, c)(v);
    f[j] = v;
  }
  Chunk8<T> o;
  o.from_f32(f);
  o.store(static_cast<T*>(d.dst) + (long)b * d.bs + sp * d.ld + cg * 8);
}

// NCDHW -> NDHWC with 4 channels per voxel (first-layer layout of pv_stem.hip): thread = voxel
template <typename S>
__global__ __launch_bounds__(kThreads) void ingest_c4_kernel(const pv_layout_desc d, long nvox) {
  const long vox = (long)blockIdx.x * kThreads + threadIdx.x;
  if (vox >= nvox) return;
  const long S3 = (long)d.T * d.H * d.W;
  const long b = vox / S3;
  const long sp = vox - b * S3;
  const IngestSrc at = ingest_src(d, sp);
  const S* src = static_cast<const S*>(d.src) + b * d.C * at.S3s + at.sps;
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = j < d.C ? ld_as_f32(src + (long)j * at.S3s) : 0.f;
    if (j < d.C && d.ch_scale) v = ingest_affine(d, j)(v);
    o[j] = (bf16_t)v;
  }
  *reinterpret_cast<bf16x4*>(static_cast<bf16_t*>(d.dst) + b * d.bs + sp * 4) = o;
}

// The same with EIGHT W-adjacent voxels per thread (the frame size is a multiple of 8 voxels and the source planes are
// 16-byte aligned: every BASELINE geometry): per channel plane one 16-byte (bf16) / 8-byte (uint8) / 2 x 16-byte
// (fp32) load instead of eight scalar ones, and 64 contiguous bytes stored -- the scalar kernel moves 2 bytes per
// load instruction and reaches 2.6 TB/s (138 us for X3D-M's 32 clips, 3.8 % of its forward).
template <typename S>
__global__ __launch_bounds__(kThreads) void ingest_c4_vec8_kernel(const pv_layout_desc d, long ngroups) {
  const long grp = (long)blockIdx.x * kThreads + threadIdx.x;
  if (grp >= ngroups) return;
  const long S3 = (long)d.T * d.H * d.W;
  const long vox = grp * 8;
  const long b = vox / S3;
  const long sp = vox - b * S3;          // multiple of 8, and so is H * W: the eight voxels share a frame
  const IngestSrc at = ingest_src(d, sp);
  const S* src = static_cast<const S*>(d.src) + b * d.C * at.S3s + at.sps;
  float f[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < d.C) {
      const S* p = src + (long)j * at.S3s;
      if constexpr (sizeof(S) == 2) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[j][i] = (float)v[i];
      } else if constexpr (sizeof(S) == 4) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[j][i] = lo[i]; f[j][4 + i] = hi[i]; }
      } else {
        typedef unsigned char u8x8 __attribute__((ext_vector_type(8)));
        const u8x8 v = *reinterpret_cast<const u8x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[j][i] = (float)v[i];
      }
      if (d.ch_scale) {
        const ChAffine k = ingest_affine(d, j);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[j][i] = k(f[j][i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[j][i] = 0.f;
    }
  }
  bf16_t* dst = static_cast<bf16_t*>(d.dst) + b * d.bs + sp * 4;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {     // two voxels = one 16-byte chunk of the first-layer layout
    const bf16x8 o = {(bf16_t)f[0][i], (bf16_t)f[1][i], (bf16_t)f[2][i], (bf16_t)f[3][i],
                      (bf16_t)f[0][i + 1], (bf16_t)f[1][i + 1], (bf16_t)f[2][i + 1], (bf16_t)f[3][i + 1]};
    *reinterpret_cast<bf16x8*>(dst + i * 4) = o;
  }
}

template <typename T, typename S>
__global__ __launch_bounds__(kThreads) void egress_kernel(const pv_layout_desc d, long nvox) {
  const int CG = d.c_p / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= nvox * CG) return;
  const long vox = id % nvox;
  const int cg = (int)(id / nvox);
  const long S3 = (long)d.T * d.H * d.W;
  const int b = (int)(vox / S3);
  const long sp = vox - (long)b * S3;
  Chunk8<T> c;
  c.load(static_cast<const T*>(d.src) + (long)b * d.bs + sp * d.ld + cg * 8);
  float f[8];
  c.to_f32(f);
  S* dst = static_cast<S*>(d.dst) + (long)b * d.C * S3 + sp;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = cg * 8 + j;
    if (ch < d.C) dst[(long)ch * S3] = (S)f[j];
  }
}

// the 4-channel first-layer layout: bf16 rows of exactly 4 channels, which the 8-channel rule below would refuse
bool layout_is_c4(const pv_layout_desc& d) {
  return d.c_p == 4 && d.ld == 4 && d.C <= 4 && d.dst_dtype == PV_BF16 && d.bs % 4 == 0;
}
bool layout_ok(const pv_layout_desc* d, bool c4_allowed) {
  if (!d || !d->src || !d->dst || d->B <= 0 || d->C <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0) return false;
  if (c4_allowed && layout_is_c4(*d)) return true;
  return !(d->c_p % 8 || d->c_p < d->C || d->ld % 8 || d->ld < d->c_p || d->bs % 8);
}

}  // namespace

extern "C" int pv_ingest_ncdhw(const pv_layout_desc* d, pv_stream_t stream) {
  if (!layout_ok(d, true) || (d->t_index && d->src_T <= 0)) return PV_ERR_INVALID;
  const long nvox = (long)d->B * d->T * d->H * d->W;
  const dim3 block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype<true>(d->src_dtype, [&](auto st) -> int {
    typedef typename decltype(st)::type S;
    if (!layout_is_c4(*d))
      return pv_for_dtype(d->dst_dtype, [&](auto dt) -> int {
        typedef typename decltype(dt)::type T;
        PV_LAUNCH((ingest_kernel<S, T>), dim3(pv_blocks(nvox * (d->c_p / 8), kThreads)), block, 0, s, *d, nvox);
        return pv_launch_status();
      });
    const long HW = (long)d->H * d->W;
    if (HW % 8 == 0 && (HW * sizeof(S)) % 16 == 0 && ((uintptr_t)d->src % 16) == 0 && ((uintptr_t)d->dst % 16) == 0 && d->bs % 8 == 0)
      PV_LAUNCH(ingest_c4_vec8_kernel<S>, dim3(pv_blocks(nvox / 8, kThreads)), block, 0, s, *d, nvox / 8);
    else
      PV_LAUNCH(ingest_c4_kernel<S>, dim3(pv_blocks(nvox, kThreads)), block, 0, s, *d, nvox);
    return pv_launch_status();
  });
}

extern "C" int pv_egress_ncdhw(const pv_layout_desc* d, pv_stream_t stream) {
  if (!layout_ok(d, false)) return PV_ERR_INVALID;
  const long nvox = (long)d->B * d->T * d->H * d->W;
  const dim3 grid(pv_blocks(nvox * (d->c_p / 8), kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // src = NDHWC side (src_dtype), dst = NCDHW side (dst_dtype)
  return pv_for_dtype(d->src_dtype, [&](auto st) -> int {
    typedef typename decltype(st)::type T;
    return pv_for_dtype(d->dst_dtype, [&](auto dt) -> int {
      typedef typename decltype(dt)::type S;
      PV_LAUNCH((egress_kernel<T, S>), grid, block, 0, s, *d, nvox);
      return pv_launch_status();
    });
  });
}
