// Row kernels of the token stream and the head: LayerNorm, BatchNorm (eval) on rows, row softmax / mean, video-level
// ensembling, positional-encoding add, residual add.  Rows are moved as 8-channel chunks (16 B of bf16), lanes over channels.
#include <float.h>
#include "pv_common.h"

namespace {

constexpr int kThreads = 256;

// --------------------------------------------------------------------- LayerNorm
// Two-pass statistics in registers.  A row is held by G lanes, each with slices of W = 8 or 4 channels; channels from C on
// hold zero.  The pieces below are the ones whose emitted code is the same through a helper.  The variance loop is
// written out in all three kernels: through a helper the compiler reuses its `x - mean` in the normalise step (fewer
// instructions in layernorm16_kernel's loop, 3 to 11 more VGPRs in layernorm_kernel), and layernorm_f32in_kernel writes
// its group sums out as well (through ln_group_sum its NL = 1 loops grow by 2 to 4 instructions).
template <int G> __device__ __forceinline__ float ln_group_sum(float v) {   // the row's G lanes; G = 64: pv_wave_sum
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the row sum, a slice at a time: 8-wide slices add in channel order, 4-wide ones pairwise
template <int W, typename V> __device__ __forceinline__ void ln_add_slice(float& s, const V& f) {
  if constexpr (W == 4) {
    s += (f[0] + f[1]) + (f[2] + f[3]);
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) s += f[j];
  }
}
__device__ __forceinline__ float ln_norm(float x, float mean, float rstd, float gamma, float beta) {
  return (x - mean) * rstd * gamma + beta;
}

// one wave per row (C <= 64*8*MAXC)
template <typename TI, typename T, int MAXC>
__global__ __launch_bounds__(kThreads) void layernorm_kernel(const pv_rows_desc d) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= d.rows) return;
  const int CG = pv_round_up(d.C, 8) / 8;
  const TI* x = static_cast<const TI*>(d.x) + row * d.ldx;
  float f[MAXC][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cg = lane + i * 64;
    if (cg < CG) {
      Chunk8<TI> c;
      c.load(x + cg * 8);
      c.to_f32(f[i]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] = 0.f;
    }
    ln_add_slice<8>(s, f[i]);   // padding channels are zero
  }
  const float mean = ln_group_sum<64>(s) / (float)d.C;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (lane + i * 64) * 8 + j;
      const float dlt = (c < d.C) ? f[i][j] - mean : 0.f;
      v += dlt * dlt;
    }
  }
  const float rstd = rsqrtf(ln_group_sum<64>(v) / (float)d.C + d.eps);
  T* y = static_cast<T*>(d.y) + row * d.ldy;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cg = lane + i * 64;
    if (cg < CG) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cg * 8 + j;
        o[j] = (c < d.C) ? ln_norm(f[i][j], mean, rstd, d.gamma ? d.gamma[c] : 1.f, d.beta ? d.beta[c] : 0.f) : 0.f;
      }
      Chunk8<T> oc;
      oc.from_f32(o);
      oc.store(y + cg * 8);
    }
  }
}

// Narrow rows (C <= 256, e.g. MViT's 96/192-wide stream and per-head norms): G = 16 or 32 lanes per
// row, 4 or 2 rows per wave, so a 96-channel row keeps 12 of 16 lanes busy instead of 12 of 64.
template <typename TI, typename T, int G>
__global__ __launch_bounds__(kThreads) void layernorm16_kernel(const pv_rows_desc d) {
  const int lane = threadIdx.x & 63;
  const int sub = lane / G, l16 = lane % G;
  const int CG = pv_round_up(d.C, 8) / 8;
  constexpr int RPW = 64 / G;                       // rows per wave per iteration
  const long wave_id = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const long wave_stride = (long)gridDim.x * (kThreads / 64);
  // this lane's slice of gamma / beta is the same for every row it will see: load it once.  With a
  // periodic table (g_period rows) that still holds, because the grid is a multiple of g_period and a
  // lane group's row index advances by multiples of 8 * gridDim.x.
  const int prow = d.g_period > 0 ? (int)((wave_id * RPW + sub) % d.g_period) * d.C : 0;
  float gm[8], bt[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = l16 * 8 + j;
    gm[j] = (c < d.C && d.gamma) ? d.gamma[prow + c] : 1.f;
    bt[j] = (c < d.C && d.beta) ? d.beta[prow + c] : 0.f;
  }
  // grid-stride over row groups, two groups in flight per wave
  for (long g0 = wave_id; g0 * RPW < d.rows; g0 += 2 * wave_stride) {
    float f[2][8];
    long row[2];
    bool act[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      row[u] = (g0 + u * wave_stride) * RPW + sub;
      act[u] = row[u] < d.rows && l16 < CG;
      if (act[u]) {
        Chunk8<TI> c;
        c.load(static_cast<const TI*>(d.x) + row[u] * d.ldx + l16 * 8);
        c.to_f32(f[u]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[u][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s = 0.f;
      ln_add_slice<8>(s, f[u]);
      const float mean = ln_group_sum<G>(s) / (float)d.C;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dlt = (l16 * 8 + j < d.C) ? f[u][j] - mean : 0.f;
        v += dlt * dlt;
      }
      const float rstd = rsqrtf(ln_group_sum<G>(v) / (float)d.C + d.eps);
      if (act[u]) {
        float o8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o8[j] = (l16 * 8 + j < d.C) ? ln_norm(f[u][j], mean, rstd, gm[j], bt[j]) : 0.f;
        Chunk8<T> oc;
        oc.from_f32(o8);
        oc.store(static_cast<T*>(d.y) + row[u] * d.ldy + l16 * 8);
      }
    }
  }
}

// fp32 rows -> `T` rows (the fp32 residual stream of the bf16 MViT plan): a lane owns FOUR channels
// (one 16-byte fp32 load, one 8-byte bf16 store), so every load instruction of a wave covers a dense
// run of memory; NL loads per lane cover rows up to 64*4*NL channels; G lanes per row.
template <typename T, int G, int NL>
__global__ __launch_bounds__(kThreads) void layernorm_f32in_kernel(const pv_rows_desc d) {
  const int lane = threadIdx.x & 63;
  const int sub = lane / G, lg = lane % G;
  constexpr int RPW = 64 / G;
  const long wave_id = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const long wave_stride = (long)gridDim.x * (kThreads / 64);
  const int C4 = pv_round_up(d.C, 8) / 4;   // 4-channel chunks per (padded) row
  f32x4 gm[NL], bt[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int c0 = (lg + i * G) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gm[i][j] = (c0 + j < d.C && d.gamma) ? d.gamma[c0 + j] : 1.f;
      bt[i][j] = (c0 + j < d.C && d.beta) ? d.beta[c0 + j] : 0.f;
    }
  }
  for (long g0 = wave_id; g0 * RPW < d.rows; g0 += 2 * wave_stride) {
    f32x4 f[2][NL];
    long row[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      row[u] = (g0 + u * wave_stride) * RPW + sub;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int ch = lg + i * G;
        if (row[u] < d.rows && ch < C4)
          f[u][i] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(d.x) + row[u] * d.ldx + ch * 4);
        else
          f[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NL; ++i) ln_add_slice<4>(s, f[u][i]);   // padding is zero
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float mean = s / (float)d.C;
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < NL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float dlt = ((lg + i * G) * 4 + j < d.C) ? f[u][i][j] - mean : 0.f;
          v += dlt * dlt;
        }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const float rstd = rsqrtf(v / (float)d.C + d.eps);
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int ch = lg + i * G;
        if (row[u] < d.rows && ch < C4) {
          float o4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o4[j] = (ch * 4 + j < d.C) ? ln_norm(f[u][i][j], mean, rstd, gm[i][j], bt[i][j]) : 0.f;
          T* yp = static_cast<T*>(d.y) + row[u] * d.ldy + ch * 4;
          if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(yp) = bf16x4{(bf16_t)o4[0], (bf16_t)o4[1], (bf16_t)o4[2], (bf16_t)o4[3]};
          else *reinterpret_cast<f32x4*>(yp) = f32x4{o4[0], o4[1], o4[2], o4[3]};
        }
      }
    }
  }
}

}  // namespace

// (not in the anonymous namespace, and never was: the kernel keeps the symbol that listings and profiles know it by)
// BatchNorm (eval) on token rows: y = act(x * gamma + beta), 8 channels per thread, rows over the grid.
// TX = float: fp32 stream in, T out (the block norms); TX = T: same type, in place allowed (the pre-pooling norm).
template <typename TX, typename T>
__global__ __launch_bounds__(kThreads) void affine_rows_kernel(const pv_rows_desc d, long total, int CG) {
  for (long id = (long)blockIdx.x * kThreads + threadIdx.x; id < total; id += (long)gridDim.x * kThreads) {
    const long row = id / CG;
    const int c0 = (int)(id - row * CG) * 8;
    const bool skip = d.rows_per_batch > 0 && (int)(row % d.rows_per_batch) < d.n_prefix;
    const TX* xp = static_cast<const TX*>(d.x) + row * d.ldx + c0;
    T* yp = static_cast<T*>(d.y) + row * d.ldy + c0;
    if (skip && static_cast<const void*>(xp) == static_cast<const void*>(yp)) continue;
    float v[8];
    Chunk8<TX> in;
    in.load(xp);
    in.to_f32(v);
    if (!skip) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = c0 + j < d.C;
        const float g = ok ? (d.gamma ? d.gamma[c0 + j] : 1.f) : 0.f;
        const float b = ok ? (d.beta ? d.beta[c0 + j] : 0.f) : 0.f;
        v[j] = v[j] * g + b;
      }
      pv_apply_act_n<sizeof(T) == 2>(v, d.act);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j >= d.C) v[j] = 0.f;
    }
    Chunk8<T> o;
    o.from_f32(v);
    o.store(yp);
  }
}

namespace {

// --------------------------------------------------------------------- softmax
// a row's maximum and 1 / sum of exp(x - max), by one wave; softmax_p is the row's probability of x
template <typename T> __device__ __forceinline__ void softmax_stats(const T* x, int C, int lane, float& mx, float& inv) {
  mx = -FLT_MAX;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, (float)x[c]);
  mx = pv_wave_max(mx);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf((float)x[c] - mx);
  s = pv_wave_sum(s);
  inv = 1.f / s;
}
__device__ __forceinline__ float softmax_p(float x, float mx, float inv) { return __expf(x - mx) * inv; }

// softmax over channels of each row (head activation); one wave per row, generic C
template <typename T>
__global__ __launch_bounds__(kThreads) void softmax_rows_kernel(const pv_rows_desc d) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= d.rows) return;
  const T* x = static_cast<const T*>(d.x) + row * d.ldx;
  T* y = static_cast<T*>(d.y) + row * d.ldy;
  float mx, inv;
  softmax_stats(x, d.C, lane, mx, inv);
  for (int c = lane; c < d.C; c += 64) y[c] = (T)softmax_p((float)x[c], mx, inv);
}

// Video-level ensembling: one wave per clip.  The wave of the FIRST clip of a video in this batch folds
// every clip of that video (in index order) into the video's score row, so no two waves touch the same
// row and the result does not depend on scheduling.
__global__ __launch_bounds__(kThreads) void ensemble_kernel(const pv_ensemble_desc d) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (i >= d.N) return;
  const int v = d.video_index[i];
  if (v < 0 || v >= d.V) return;
  for (int j = 0; j < i; ++j)
    if (d.video_index[j] == v) return;   // an earlier clip's wave owns this video
  float* acc = d.accum + (long)v * d.C;
  int cnt = 0;
  for (int j = i; j < d.N; ++j) {
    if (d.video_index[j] != v) continue;
    const float* x = d.logits + (long)j * d.ld;
    float mx, inv;
    softmax_stats(x, d.C, lane, mx, inv);
    for (int c = lane; c < d.C; c += 64) {
      const float p = softmax_p(x[c], mx, inv);
      acc[c] = d.mode == 1 ? fmaxf(acc[c], p) : acc[c] + p;   // same lane re-reads what it wrote: ordered
    }
    ++cnt;
  }
  if (lane == 0) d.counts[v] += cnt;
}

// --------------------------------------------------------------------- mean, positional encoding, residual add
// y[b][c] = mean over rows_per_batch rows (fp32 out); thread per (b, c)
template <typename T>
__global__ __launch_bounds__(kThreads) void mean_rows_kernel(const pv_rows_desc d, int nb) {
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (long)nb * d.C) return;
  const int c = (int)(id % d.C);
  const int b = (int)(id / d.C);
  const T* x = static_cast<const T*>(d.x) + (long)b * d.rows_per_batch * d.ldx + c;
  float s = 0.f;
  for (int r = 0; r < d.rows_per_batch; ++r) s += (float)x[(long)r * d.ldx];
  static_cast<float*>(d.y)[(long)b * d.ldy + c] = s / (float)d.rows_per_batch;
}

// tokens[b][0] = cls + pos_class ; tokens[b][1+t*HW+s] += pos_spatial[s] + pos_temporal[t]
template <typename T>
__global__ __launch_bounds__(kThreads) void posenc_kernel(const pv_posenc_desc d, long total) {
  const int c_p = pv_round_up(d.C, 8);
  const int CG = c_p / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= total) return;
  const int cg = (int)(id % CG);
  long r = id / CG;
  const int has_cls = d.cls_token != nullptr;
  const long rows = (long)d.T * d.HW + has_cls;
  const int b = d.cls_only ? (int)r : (int)(r / rows);          // cls_only: one work item per (clip, chunk)
  const long n = d.cls_only ? 0 : r - (long)b * rows;
  T* x = static_cast<T*>(d.x) + ((long)b * rows + n) * d.ld + cg * 8;
  float f[8];
  if (has_cls && n == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cg * 8 + j;
      float v = 0.f;
      if (c < d.C) {
        v = d.cls_token[c];
        if (d.pos_temporal != nullptr) { if (d.pos_class) v += d.pos_class[c]; }
        else v += d.pos_spatial[c];  // full table: row 0 belongs to cls
      }
      f[j] = v;
    }
  } else {
    Chunk8<T> cch;
    cch.load(x);
    cch.to_f32(f);
    const long g = n - has_cls;
    const int t = (int)(g / d.HW), s = (int)(g - (long)t * d.HW);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cg * 8 + j;
      if (c < d.C) {
        if (d.pos_temporal != nullptr)
          f[j] += d.pos_spatial[(long)s * d.C + c] + d.pos_temporal[(long)t * d.C + c];
        else
          f[j] += d.pos_spatial[(g + has_cls) * d.C + c];
      }
    }
  }
  Chunk8<T> o;
  o.from_f32(f);
  o.store(x);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void add_act_kernel(const pv_add_desc d, long total) {
  const int CG = pv_round_up(d.C, 8) / 8;
  const long id = (long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= total) return;
  const int cg = (int)(id % CG);
  const long r = id / CG;
  Chunk8<T> a, b;
  a.load(static_cast<const T*>(d.a) + r * d.lda + cg * 8);
  b.load(static_cast<const T*>(d.b) + r * d.ldb + cg * 8);
  float fa[8], fb[8];
  a.to_f32(fa);
  b.to_f32(fb);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    fa[j] = pv_apply_act(fa[j] + fb[j], d.act);
    if (cg * 8 + j >= d.C) fa[j] = 0.f;
  }
  a.from_f32(fa);
  a.store(static_cast<T*>(d.y) + r * d.ldy + cg * 8);
}

// --------------------------------------------------------------------- host side
bool rows_ok(const pv_rows_desc* d) { return d && d->x && d->y && d->rows > 0 && d->C > 0; }

// the kernels with G lanes per row: a wave takes 64 / G rows at a time, two such groups in flight
dim3 ln_group_grid(const pv_rows_desc& d, int G) {
  long nb = pv_ceil_div(d.rows, (kThreads / 64) * (64 / G) * 2);
  nb = nb < 4096 ? nb : 4096;
  if (d.g_period > 1) nb = pv_ceil_div(nb, d.g_period) * d.g_period;   // layernorm16_kernel's gamma / beta rows
  return dim3((unsigned)nb);
}
template <typename T, int G> int ln16_launch(const pv_rows_desc& d, hipStream_t s) {
  PV_LAUNCH((layernorm16_kernel<T, T, G>), ln_group_grid(d, G), dim3(kThreads), 0, s, d);
  return pv_launch_status();
}
template <int G, int NL> int ln_f32in_launch(const pv_rows_desc& d, hipStream_t s) {
  PV_LAUNCH((layernorm_f32in_kernel<bf16_t, G, NL>), ln_group_grid(d, G), dim3(kThreads), 0, s, d);
  return pv_launch_status();
}
template <typename TI, typename T, int MAXC> int ln_launch(const pv_rows_desc& d, hipStream_t s) {
  PV_LAUNCH((layernorm_kernel<TI, T, MAXC>), dim3((unsigned)pv_ceil_div(d.rows, kThreads / 64)), dim3(kThreads), 0, s, d);
  return pv_launch_status();
}

}  // namespace

extern "C" int pv_layernorm(const pv_rows_desc* d, pv_stream_t stream) {
  if (!rows_ok(d)) return PV_ERR_INVALID;
  if (d->ldx % 8 || d->ldy % 8) return PV_ERR_INVALID;
  const int CG = pv_round_up(d->C, 8) / 8;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->g_period < 0 || d->g_period > 16) return PV_ERR_INVALID;
  if (d->g_period > 1 && (CG > 32 || d->x_f32 || 16 % d->g_period)) return PV_ERR_UNSUPPORTED;   // narrow-row kernel only
  if (d->dtype == PV_BF16 && d->x_f32) {   // fp32 stream -> bf16 operand: 4 channels per lane up to 1024 channels
    const int C4 = CG * 2;
    if (C4 <= 16) return ln_f32in_launch<16, 1>(*d, s);
    if (C4 <= 32) return ln_f32in_launch<32, 1>(*d, s);
    if (C4 <= 64) return ln_f32in_launch<64, 1>(*d, s);
    if (C4 <= 128) return ln_f32in_launch<64, 2>(*d, s);
    if (C4 <= 256) return ln_f32in_launch<64, 4>(*d, s);
    return CG <= 256 ? ln_launch<float, bf16_t, 4>(*d, s) : PV_ERR_UNSUPPORTED;
  }
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    typedef typename decltype(t)::type T;
    if (CG <= 16) return ln16_launch<T, 16>(*d, s);
    if (CG <= 32) return ln16_launch<T, 32>(*d, s);
    if (CG <= 64) return ln_launch<T, T, 1>(*d, s);
    if (CG <= 128) return ln_launch<T, T, 2>(*d, s);
    return CG <= 256 ? ln_launch<T, T, 4>(*d, s) : PV_ERR_UNSUPPORTED;
  });
}

extern "C" int pv_affine_rows(const pv_rows_desc* d, pv_stream_t stream) {
  if (!rows_ok(d)) return PV_ERR_INVALID;
  if (d->ldx % 8 || d->ldy % 8 || d->g_period != 0 || d->n_prefix < 0 || d->rows_per_batch < 0) return PV_ERR_INVALID;
  if (d->n_prefix > 0 && d->rows_per_batch <= 0) return PV_ERR_INVALID;
  const int CG = pv_round_up(d->C, 8) / 8;
  const long total = d->rows * CG;
  long nb = pv_ceil_div(total, kThreads);
  nb = nb < 8192 ? nb : 8192;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid((unsigned)nb), block(kThreads);
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    typedef typename decltype(t)::type T;
    if (d->x_f32) PV_LAUNCH((affine_rows_kernel<float, T>), grid, block, 0, s, *d, total, CG);
    else PV_LAUNCH((affine_rows_kernel<T, T>), grid, block, 0, s, *d, total, CG);
    return pv_launch_status();
  });
}

extern "C" int pv_softmax_rows(const pv_rows_desc* d, pv_stream_t stream) {
  if (!rows_ok(d)) return PV_ERR_INVALID;
  dim3 grid((unsigned)pv_ceil_div(d->rows, kThreads / 64)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    PV_LAUNCH(softmax_rows_kernel<typename decltype(t)::type>, grid, block, 0, s, *d);
    return pv_launch_status();
  });
}

extern "C" int pv_ensemble_scores(const pv_ensemble_desc* d, pv_stream_t stream) {
  if (!d || !d->logits || !d->video_index || !d->accum || !d->counts) return PV_ERR_INVALID;
  if (d->N <= 0 || d->C <= 0 || d->V <= 0 || d->ld < d->C || (d->mode != 0 && d->mode != 1)) return PV_ERR_INVALID;
  PV_LAUNCH(ensemble_kernel, dim3((unsigned)pv_ceil_div(d->N, kThreads / 64)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), *d);
  return pv_launch_status();
}

extern "C" int pv_mean_rows(const pv_rows_desc* d, pv_stream_t stream) {
  if (!rows_ok(d)) return PV_ERR_INVALID;
  if (d->rows_per_batch <= 0 || d->rows % d->rows_per_batch) return PV_ERR_INVALID;
  const int nb = (int)(d->rows / d->rows_per_batch);
  dim3 grid(pv_blocks((long)nb * d->C, kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    PV_LAUNCH(mean_rows_kernel<typename decltype(t)::type>, grid, block, 0, s, *d, nb);
    return pv_launch_status();
  });
}

extern "C" int pv_add_posenc(const pv_posenc_desc* d, pv_stream_t stream) {
  if (!d || !d->x || !d->pos_spatial) return PV_ERR_INVALID;
  if (d->B <= 0 || d->T <= 0 || d->HW <= 0 || d->C <= 0 || d->ld % 8) return PV_ERR_INVALID;
  const long rows = (long)d->T * d->HW + (d->cls_token ? 1 : 0);
  if (d->cls_only && !d->cls_token) return PV_ERR_INVALID;
  const long total = (long)d->B * (d->cls_only ? 1 : rows) * (pv_round_up(d->C, 8) / 8);
  dim3 grid(pv_blocks(total, kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    PV_LAUNCH(posenc_kernel<typename decltype(t)::type>, grid, block, 0, s, *d, total);
    return pv_launch_status();
  });
}

extern "C" int pv_add_act(const pv_add_desc* d, pv_stream_t stream) {
  if (!d || !d->a || !d->b || !d->y || d->rows <= 0 || d->C <= 0) return PV_ERR_INVALID;
  if (d->lda % 8 || d->ldb % 8 || d->ldy % 8) return PV_ERR_INVALID;
  const long total = d->rows * (pv_round_up(d->C, 8) / 8);
  dim3 grid(pv_blocks(total, kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pv_for_dtype(d->dtype, [&](auto t) -> int {
    PV_LAUNCH(add_act_kernel<typename decltype(t)::type>, grid, block, 0, s, *d, total);
    return pv_launch_status();
  });
}
