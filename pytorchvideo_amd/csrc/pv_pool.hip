// Max / average pooling over NDHWC rows (count_include_pad=True), 8-channel chunks (16 B of bf16) with lanes running over
// channels first: small windows one thread per (output voxel, chunk), large windows one block per output voxel.
#include <float.h>
#include "pv_common.h"

namespace {

constexpr int kThreads = 256;

// ---- the stages every kernel has: which output voxel, where its item's input starts, the neutral element, the result ----
struct PoolVoxel { int b, to, ho, wo; };
__device__ __forceinline__ PoolVoxel pool_voxel(const pv_pool3d_desc& d, long v) {
  PoolVoxel o;
  o.wo = (int)(v % d.Wo); v /= d.Wo;
  o.ho = (int)(v % d.Ho); v /= d.Ho;
  o.to = (int)(v % d.To);
  o.b = (int)(v / d.To);
  return o;
}
// chunk cg of the first voxel behind the prefix rows of item b
template <typename T> __device__ __forceinline__ const T* pool_src(const pv_pool3d_desc& d, int b, int cg) {
  return static_cast<const T*>(d.x) + (long)b * d.x_bs + (long)d.n_prefix * d.ldx + cg * 8;
}
__device__ __forceinline__ void pool_init(float (&a)[8], bool is_max) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = is_max ? -FLT_MAX : 0.f;
}
// an average is the sum over `taps` (count_include_pad=True); padding channels are stored as zero
template <typename T>
__device__ __forceinline__ void pool_finish(const pv_pool3d_desc& d, const PoolVoxel& o, int cg, bool is_max, int taps, float (&a)[8]) {
  if (!is_max) {
    const float inv = 1.f / (float)taps;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= inv;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (cg * 8 + j >= d.C) a[j] = 0.f;
  Chunk8<T> c;
  c.from_f32(a);
  c.store(static_cast<T*>(d.y) + (long)o.b * d.y_bs + (long)d.n_prefix * d.ldy +
          ((long)(o.to * d.Ho + o.ho) * d.Wo + o.wo) * d.ldy + cg * 8);
}

// small windows: one thread per (output voxel, chunk)
template <typename T>
__global__ __launch_bounds__(kThreads) void pool_direct_kernel(const pv_pool3d_desc d, long total) {
  const int CG = pv_round_up(d.C, 8) / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= total) return;
  const int cg = (int)(id % CG);
  const PoolVoxel o = pool_voxel(d, id / CG);
  const T* X = pool_src<T>(d, o.b, cg);
  float a[8];
  const bool is_max = d.mode == PV_POOL_MAX;
  pool_init(a, is_max);
  for (int dt = 0; dt < d.kt; ++dt) {
    const int ti = o.to * d.st - d.pt + dt;
    if ((unsigned)ti >= (unsigned)d.Ti) continue;
    for (int dh = 0; dh < d.kh; ++dh) {
      const int hi = o.ho * d.sh - d.ph + dh;
      if ((unsigned)hi >= (unsigned)d.Hi) continue;
      for (int dw = 0; dw < d.kw; ++dw) {
        const int wi = o.wo * d.sw - d.pw + dw;
        if ((unsigned)wi >= (unsigned)d.Wi) continue;
        Chunk8<T> c;
        c.load(X + ((long)(ti * d.Hi + hi) * d.Wi + wi) * d.ldx);
        float f[8];
        c.to_f32(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = is_max ? fmaxf(a[j], f[j]) : a[j] + f[j];
      }
    }
  }
  pool_finish<T>(d, o, cg, is_max, d.kt * d.kh * d.kw, a);
}

// The windows the models use between layers -- 3x3x3 (MViT's skip-path max pool, layers/attention.py:677-679,720-727) and
// 1x3x3 (SlowFast / ResNet stem pools, models/stem.py:98-104) -- with the taps unrolled: every load of a temporal slice is issued
// unconditionally from a clamped address (no branch per tap: the runtime loops above wait for each load behind its own bounds
// test), validity is applied as a select.  One output voxel x 8-channel chunk per thread, as above.
template <typename T, int KT, int KH, int KW>
__global__ __launch_bounds__(kThreads) void pool_window_kernel(const pv_pool3d_desc d, long total) {
  const int CG = pv_round_up(d.C, 8) / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= total) return;
  const int cg = (int)(id % CG);
  const PoolVoxel o = pool_voxel(d, id / CG);
  const T* X = pool_src<T>(d, o.b, cg);
  const bool is_max = d.mode == PV_POOL_MAX;
  float a[8];
  pool_init(a, is_max);
  const int h0 = o.ho * d.sh - d.ph, w0 = o.wo * d.sw - d.pw;
  int hoff[KH], woff[KW];
  bool hok[KH], wok[KW];
#pragma unroll
  for (int dh = 0; dh < KH; ++dh) {
    const int hi = h0 + dh;
    hok[dh] = (unsigned)hi < (unsigned)d.Hi;
    hoff[dh] = (hok[dh] ? hi : 0) * d.Wi;
  }
#pragma unroll
  for (int dw = 0; dw < KW; ++dw) {
    const int wi = w0 + dw;
    wok[dw] = (unsigned)wi < (unsigned)d.Wi;
    woff[dw] = wok[dw] ? wi : 0;
  }
#pragma unroll
  for (int dt = 0; dt < KT; ++dt) {
    const int ti = o.to * d.st - d.pt + dt;
    const bool tok = (unsigned)ti < (unsigned)d.Ti;
    const T* P = X + (long)(tok ? ti : 0) * d.Hi * d.Wi * d.ldx;
    Chunk8<T> c[KH][KW];
#pragma unroll
    for (int dh = 0; dh < KH; ++dh)
#pragma unroll
      for (int dw = 0; dw < KW; ++dw) c[dh][dw].load(P + (long)(hoff[dh] + woff[dw]) * d.ldx);
#pragma unroll
    for (int dh = 0; dh < KH; ++dh)
#pragma unroll
      for (int dw = 0; dw < KW; ++dw) {
        const bool ok = tok && hok[dh] && wok[dw];
        float f[8];
        c[dh][dw].to_f32(f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = is_max ? fmaxf(a[j], ok ? f[j] : -FLT_MAX) : a[j] + (ok ? f[j] : 0.f);
      }
  }
  pool_finish<T>(d, o, cg, is_max, KT * KH * KW, a);
}

// large windows: one block per output voxel (and chunk slab), taps split over threads.
// A thread's taps sp, sp + splits, ... go out kPoolBatch at a time as straight-line code, all loads of a batch ahead of
// its additions, and are accumulated in tap order.  Nothing is divided or multiplied per tap: the tap's byte offset steps
// with it -- by a constant where the window is a run of whole input planes (WHOLE: the head pools, tap t is voxel
// t0 * Hi * Wi + t), with (dt, dh, dw) and their carries otherwise.  A tap outside the input loads the item's first voxel
// instead and contributes the neutral element; so does, in the thread's last batch, a tap past the window's end.
constexpr int kPoolBatch = 8;
template <bool B> struct BoolC { static constexpr bool value = B; };
template <typename T, bool MAX, bool WHOLE>
__device__ __forceinline__ void pool_reduce_taps(const pv_pool3d_desc& d, const T* X, int t0, int h0, int w0, int sp,
                                                 int splits, int taps, float (&a)[8]) {
  const long vox = (long)d.ldx * (long)sizeof(T), row = vox * d.Wi, plane = row * d.Hi;   // bytes
  int dt = 0, dh = 0, dw = 0, s_t = 0, s_h = 0, s_w = 0;
  long off, step, wrap_w = 0, wrap_h = 0;
  if (WHOLE) {
    off = t0 * plane + sp * vox;
    step = splits * vox;
  } else {
    const int khw = d.kh * d.kw;
    s_t = splits / khw;
    s_h = (splits - s_t * khw) / d.kw;
    s_w = splits - s_t * khw - s_h * d.kw;
    dt = sp / khw;
    dh = (sp - dt * khw) / d.kw;
    dw = sp - dt * khw - dh * d.kw;
    off = (t0 + dt) * plane + (h0 + dh) * row + (w0 + dw) * vox;
    step = s_t * plane + s_h * row + s_w * vox;
    wrap_w = row - d.kw * vox;       // dw -= kw, ++dh
    wrap_h = plane - d.kh * row;     // dh -= kh, ++dt
  }
  const char* Xb = reinterpret_cast<const char*>(X);
  const float neutral = MAX ? -FLT_MAX : 0.f;
  int t = sp;
  auto batch = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;     // every tap of the batch is inside the window
    Chunk8<T> c[kPoolBatch];
    bool ok[kPoolBatch];
#pragma unroll
    for (int i = 0; i < kPoolBatch; ++i) {
      ok[i] = FULL || t + i * splits < taps;
      if (!WHOLE)
        ok[i] = ok[i] && (unsigned)(t0 + dt) < (unsigned)d.Ti && (unsigned)(h0 + dh) < (unsigned)d.Hi &&
                (unsigned)(w0 + dw) < (unsigned)d.Wi;
      c[i].load(reinterpret_cast<const T*>(Xb + (ok[i] ? off : 0L)));
      off += step;
      if (!WHOLE) {
        dw += s_w;
        if (dw >= d.kw) { dw -= d.kw; ++dh; off += wrap_w; }
        dh += s_h;
        if (dh >= d.kh) { dh -= d.kh; ++dt; off += wrap_h; }
        dt += s_t;
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the batch's loads together: sunk to their uses, each is waited for alone
#pragma unroll
    for (int i = 0; i < kPoolBatch; ++i) {
      float f[8];
      c[i].to_f32(f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = ok[i] ? f[j] : neutral;
        a[j] = MAX ? fmaxf(a[j], v) : a[j] + v;
      }
    }
    t += kPoolBatch * splits;
  };
  while (t + (kPoolBatch - 1) * splits < taps) batch(BoolC<true>());
  if (t < taps) batch(BoolC<false>());
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pool_reduce_kernel(const pv_pool3d_desc d, int cgb) {
  __shared__ float s_red[kThreads * 8];
  const int CG = pv_round_up(d.C, 8) / 8;
  const int tid = threadIdx.x;
  const int splits = kThreads / cgb;
  const int cgl = tid % cgb, sp = tid / cgb;
  const int cg = blockIdx.y * cgb + cgl;
  const PoolVoxel o = pool_voxel(d, blockIdx.x);
  const bool is_max = d.mode == PV_POOL_MAX;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = is_max ? -FLT_MAX : 0.f;   // pool_init, written out (as pool_finish below)
  const int taps = d.kt * d.kh * d.kw;
  if (cg < CG && sp < splits) {
    const T* X = pool_src<T>(d, o.b, cg);
    const int t0 = o.to * d.st - d.pt, h0 = o.ho * d.sh - d.ph, w0 = o.wo * d.sw - d.pw;
    const bool whole = t0 >= 0 && t0 + d.kt <= d.Ti && h0 == 0 && d.kh == d.Hi && w0 == 0 && d.kw == d.Wi;
    if (is_max) {
      if (whole) pool_reduce_taps<T, true, true>(d, X, t0, h0, w0, sp, splits, taps, a);
      else pool_reduce_taps<T, true, false>(d, X, t0, h0, w0, sp, splits, taps, a);
    } else {
      if (whole) pool_reduce_taps<T, false, true>(d, X, t0, h0, w0, sp, splits, taps, a);
      else pool_reduce_taps<T, false, false>(d, X, t0, h0, w0, sp, splits, taps, a);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[tid * 8 + j] = a[j];
  __syncthreads();
  if (sp == 0 && cg < CG) {
    for (int s2 = 1; s2 < splits; ++s2) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = s_red[(s2 * cgb + cgl) * 8 + j];
        a[j] = is_max ? fmaxf(a[j], v) : a[j] + v;
      }
    }
    // pool_finish and pool_init, written out: this kernel runs at its launch floor, and through the helpers its code
    // changes (the bf16 finish takes 9 more instructions, pool_init renumbers the registers of the whole tap walk)
    if (!is_max) {
      const float inv = 1.f / (float)taps;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] *= inv;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (cg * 8 + j >= d.C) a[j] = 0.f;
    Chunk8<T> c;
    c.from_f32(a);
    c.store(static_cast<T*>(d.y) + (long)o.b * d.y_bs + (long)d.n_prefix * d.ldy +
            ((long)(o.to * d.Ho + o.ho) * d.Wo + o.wo) * d.ldy + cg * 8);
  }
}

// copy the n_prefix leading rows (cls token) of every batch item
template <typename T>
__global__ void pool_prefix_kernel(const pv_pool3d_desc d) {
  const int CG = pv_round_up(d.C, 8) / 8;
  const int total = d.B * d.n_prefix * CG;
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const int cg = id % CG;
  const int r = (id / CG) % d.n_prefix;
  const int b = id / (CG * d.n_prefix);
  Chunk8<T> c;
  c.load(static_cast<const T*>(d.x) + (long)b * d.x_bs + (long)r * d.ldx + cg * 8);
  c.store(static_cast<T*>(d.y) + (long)b * d.y_bs + (long)r * d.ldy + cg * 8);
}

template <typename T> int pool_launch(const pv_pool3d_desc& d, hipStream_t s) {
  const int CG = pv_round_up(d.C, 8) / 8;
  const int taps = d.kt * d.kh * d.kw;
  const long nvox = (long)d.B * d.To * d.Ho * d.Wo;
  if (taps >= 64) {
    // 8 chunks (128 contiguous bytes of a voxel) per block, the window split 32 ways: the head pools
    // (16x7x7 over 432 channels, 8x7x7 over 2048) have only B..4B output voxels, so the parallelism has
    // to come from the channel slabs and the taps
    const int cgb = CG < 8 ? CG : 8;
    if (nvox > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
    dim3 grid((unsigned)nvox, (unsigned)pv_ceil_div(CG, cgb));
    PV_LAUNCH(pool_reduce_kernel<T>, grid, dim3(kThreads), 0, s, d, cgb);
  } else {
    const long total = nvox * CG;
    const dim3 grid(pv_blocks(total, kThreads)), block(kThreads);
    const bool win = pv_tune("pool_window", 1) != 0;
    if (win && d.kt == 3 && d.kh == 3 && d.kw == 3) PV_LAUNCH((pool_window_kernel<T, 3, 3, 3>), grid, block, 0, s, d, total);
    else if (win && d.kt == 1 && d.kh == 3 && d.kw == 3) PV_LAUNCH((pool_window_kernel<T, 1, 3, 3>), grid, block, 0, s, d, total);
    else PV_LAUNCH(pool_direct_kernel<T>, grid, block, 0, s, d, total);
  }
  PV_LAUNCH_CHECK();
  if (d.n_prefix > 0) {
    const int total = d.B * d.n_prefix * CG;
    PV_LAUNCH(pool_prefix_kernel<T>, dim3(pv_blocks(total, kThreads)), dim3(kThreads), 0, s, d);
    PV_LAUNCH_CHECK();
  }
  return PV_OK;
}

}  // namespace

extern "C" int pv_pool3d(const pv_pool3d_desc* dp, pv_stream_t stream) {
  if (!dp || !dp->x || !dp->y) return PV_ERR_INVALID;
  const pv_pool3d_desc& d = *dp;
  if (d.B <= 0 || d.C <= 0 || d.To <= 0 || d.Ho <= 0 || d.Wo <= 0) return PV_ERR_INVALID;
  if (d.ldx % 8 || d.ldy % 8 || d.x_bs % 8 || d.y_bs % 8) return PV_ERR_INVALID;
  if (d.kt < 1 || d.kh < 1 || d.kw < 1 || d.st < 1 || d.sh < 1 || d.sw < 1) return PV_ERR_INVALID;
  if ((d.Ti + 2 * d.pt - d.kt) / d.st + 1 != d.To || (d.Hi + 2 * d.ph - d.kh) / d.sh + 1 != d.Ho ||
      (d.Wi + 2 * d.pw - d.kw) / d.sw + 1 != d.Wo)
    return PV_ERR_INVALID;
  if (d.mode != PV_POOL_MAX && d.mode != PV_POOL_AVG) return PV_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype(d.dtype, [&](auto t) -> int { return pool_launch<typename decltype(t)::type>(d, s); });
}
