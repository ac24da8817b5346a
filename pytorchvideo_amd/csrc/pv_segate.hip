// Squeeze-excitation gate: psum[b][blk][c_p] (per-tile channel sums left by the depthwise conv) -> gate[b][c_p]
// = sigmoid(fc2(relu(fc1(mean)))).  One block per batch item; a generic kernel and one for the sizes X3D uses.
#include "pv_common.h"

namespace {

constexpr int kThreads = 256;

// The mean's first stage, shared so that both kernels add in one order: the rows of the partial-sum table are split over
// `groups` = kThreads / cw groups of the first kThreads threads (cw: channels covered per pass); each group walks its rows with
// coalesced loads over the channels (4 independent loads in flight per thread) and leaves its sum in s_part[g][c].
__host__ __device__ __forceinline__ int se_cw(int c_p) { return c_p < kThreads ? c_p : kThreads; }
__device__ __forceinline__ void se_partial_sums(const pv_se_gate_desc& d, int b, int tid, int cw, int groups, float* s_part) {
  const float* ps = d.psum + (long)b * d.nblk * d.c_p;
  const int g = tid / cw, cl = tid - g * cw;
  for (int c0 = 0; c0 < d.c_p; c0 += cw) {
    const int c = c0 + cl;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (g < groups && c < d.c_p) {
      int k = g;
      for (; k + 3 * groups < d.nblk; k += 4 * groups) {
        a0 += ps[(long)k * d.c_p + c];
        a1 += ps[(long)(k + groups) * d.c_p + c];
        a2 += ps[(long)(k + 2 * groups) * d.c_p + c];
        a3 += ps[(long)(k + 3 * groups) * d.c_p + c];
      }
      for (; k < d.nblk; k += groups) a0 += ps[(long)k * d.c_p + c];
      s_part[g * d.c_p + c] = (a0 + a1) + (a2 + a3);
    }
  }
}

__global__ __launch_bounds__(kThreads) void se_gate_kernel(const pv_se_gate_desc d) {
  extern __shared__ float s[];
  float* s_mean = s;                 // [c_p]
  float* s_hid = s + d.c_p;          // [cr]
  float* s_part = s + d.c_p + d.cr;  // [groups][c_p]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cw = se_cw(d.c_p);
  const int groups = kThreads / cw;
  se_partial_sums(d, b, tid, cw, groups, s_part);
  __syncthreads();
  for (int c = tid; c < d.c_p; c += kThreads) {
    float a = 0.f;
    for (int gg = 0; gg < groups; ++gg) a += s_part[gg * d.c_p + c];
    s_mean[c] = a * d.inv_count;
  }
  __syncthreads();
  // fc1 + relu: one wave per hidden unit
  const int lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < d.cr; r += kThreads / 64) {
    float a = 0.f;
    for (int c = lane; c < d.C; c += 64) a += d.w1[(long)r * d.C + c] * s_mean[c];
    a = pv_wave_sum(a);
    if (lane == 0) s_hid[r] = fmaxf(a + (d.b1 ? d.b1[r] : 0.f), 0.f);
  }
  __syncthreads();
  for (int c = tid; c < d.c_p; c += kThreads) {
    float g2 = 0.f;
    if (c < d.C) {
      float a = d.b2 ? d.b2[c] : 0.f;
      for (int r = 0; r < d.cr; ++r) a += d.w2[(long)c * d.cr + r] * s_hid[r];
      g2 = pv_sigmoid(a);
    }
    d.gate[(long)b * d.c_p + c] = g2;
  }
}

// The same gate for the sizes X3D uses (C <= 448, reduced width <= 32): this kernel is a chain of four
// dependent phases on a handful of bytes, so its duration is the sum of their memory latencies and of the
// instructions one wave has to issue between them.  Every FC weight a thread will need is requested at kernel
// entry, together with the first partial sums, so the phases after the first run out of registers and LDS.
// fc2's matrix is [C][cr], and thread = channel would fetch it with one dword load per hidden unit, the 64
// lanes of a wave in 64 different lines (at C = 432, cr = 32 about 16 k line requests per workgroup for
// 55 KB that are contiguous in memory).  The block therefore fetches w2 as the flat array it is, 16 bytes
// per lane, and spreads it into an LDS image [C][cr | 1]: the odd pitch puts the rows that the lanes of a
// wave read in fc2 on different banks.
// The wider stages run more waves (se_threads): the mean keeps the 256-thread split of the rows, on which the
// order of its sum depends; fc1 (one wave per hidden unit), fc2 (one thread per channel) and the staging of w2
// do the same arithmetic whichever wave does it, and each wave has a quarter of the instructions to issue.
constexpr int kSeMaxCp = 512;   // channels (padded) the fast kernel covers
__host__ __device__ constexpr int se_threads(int cj, int crp) { return cj * crp > 64 ? 1024 : cj * crp > 16 ? 512 : kThreads; }
__host__ __device__ __forceinline__ int se_w2_pitch(int cr) { return cr | 1; }
// floats of dynamic LDS: s_mean[c_p], s_hid[32], s_part[groups][c_p], s_w2[C][pitch] + 32 (fc2 reads CRP <= 32
// columns of every row unconditionally, so the last row's reads end inside the allocation)
__host__ __device__ __forceinline__ int se_w2_lds_off(int c_p, int groups) { return c_p + 32 + groups * c_p; }
// CJ: 64-channel strides covering C (<= 7); CRP: reduced width rounded up to 8 / 16 / 32
template <int CJ, int CRP>
__global__ __launch_bounds__(se_threads(CJ, CRP)) void se_gate_fast_kernel(const pv_se_gate_desc d) {
  constexpr int NT = se_threads(CJ, CRP);
  constexpr int kSeMaxC64 = CJ;
  constexpr int kSeMaxR = CRP / (NT / 64);                          // hidden units per wave
  constexpr int kSeMaxCh = kSeMaxCp / NT > 0 ? kSeMaxCp / NT : 1;   // channels per thread
  constexpr int kW2Q = (CJ * 64 * CRP / 4 + NT - 1) / NT;           // 16-byte pieces of w2 per thread
  extern __shared__ float s[];
  float* s_mean = s;                 // [c_p]
  float* s_hid = s + d.c_p;          // [32]
  float* s_part = s + d.c_p + 32;    // [groups][c_p]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int cw = se_cw(d.c_p);
  const int groups = kThreads / cw;
  float* s_w2 = s + se_w2_lds_off(d.c_p, groups);   // [C][pitch]
  // ---- prefetch: fc2 matrix (flat, to LDS below), fc1 rows (wave = hidden unit), biases ----
  // w2 = `head` leading floats up to the first 16-byte boundary, nq aligned 16-byte pieces, a tail of < 4 floats
  const int n2 = d.C * d.cr;
  int head = (int)((16u - (unsigned)((size_t)d.w2 & 15u)) & 15u) >> 2;
  head = head < n2 ? head : n2;
  const int nq = (n2 - head) >> 2;
  const int ntail = n2 - head - 4 * nq;
  f32x4 w2q[kW2Q];
#pragma unroll
  for (int i = 0; i < kW2Q; ++i) {
    const int q = tid + i * NT;
    w2q[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < nq) w2q[i] = *reinterpret_cast<const f32x4*>(d.w2 + head + 4 * q);
  }
  // the ragged ends: threads 0..2 take the head, threads 4..6 the tail
  const int e_rag = tid < 4 ? (tid < head ? tid : -1) : (tid - 4 < ntail ? head + 4 * nq + tid - 4 : -1);
  float w2rag = 0.f;
  if (e_rag >= 0) w2rag = d.w2[e_rag];
  float w1r[kSeMaxR][kSeMaxC64], b1r[kSeMaxR];
#pragma unroll
  for (int i = 0; i < kSeMaxR; ++i) {
    const int r = wave + i * (NT / 64);
    const bool rok = r < d.cr;
    b1r[i] = (rok && d.b1) ? d.b1[r] : 0.f;
#pragma unroll
    for (int j = 0; j < kSeMaxC64; ++j) {
      const int c = lane + j * 64;
      const bool ok = rok && c < d.C;
      const float v = d.w1[ok ? (long)r * d.C + c : 0];
      w1r[i][j] = ok ? v : 0.f;
    }
  }
  float b2r[kSeMaxCh];
#pragma unroll
  for (int i = 0; i < kSeMaxCh; ++i) {
    const int c = tid + i * NT;
    b2r[i] = (c < d.C && d.b2) ? d.b2[c] : 0.f;
  }
  // ---- mean over T,H,W from the per-tile partial sums: the first kThreads threads, as the generic kernel ----
  se_partial_sums(d, b, tid, cw, groups, s_part);
  // ---- w2 into its LDS image: element e of the flat array is row e / cr, column e % cr; a thread's
  // pieces are 4 * NT elements apart, so it divides once and steps (row, column) from piece to piece ----
  {
    const int pitch = se_w2_pitch(d.cr);
    const int e0 = head + 4 * tid;
    int row = e0 / d.cr, col = e0 - row * d.cr;
    const int srow = 4 * NT / d.cr, scol = 4 * NT - srow * d.cr;
#pragma unroll
    for (int i = 0; i < kW2Q; ++i) {
      int r = row, c = col;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (tid + i * NT < nq) s_w2[r * pitch + c] = w2q[i][k];
        if (++c == d.cr) { c = 0; ++r; }
      }
      row += srow;
      col += scol;
      if (col >= d.cr) { col -= d.cr; ++row; }
    }
    if (e_rag >= 0) {
      const int r = e_rag / d.cr;
      s_w2[r * pitch + (e_rag - r * d.cr)] = w2rag;
    }
  }
  __syncthreads();
  for (int c = tid; c < d.c_p; c += NT) {
    float a = 0.f;
    for (int gg = 0; gg < groups; ++gg) a += s_part[gg * d.c_p + c];
    s_mean[c] = a * d.inv_count;
  }
  __syncthreads();
  // ---- fc1 + relu ----
  float mj[kSeMaxC64];
#pragma unroll
  for (int j = 0; j < kSeMaxC64; ++j) mj[j] = lane + j * 64 < d.C ? s_mean[lane + j * 64] : 0.f;
#pragma unroll
  for (int i = 0; i < kSeMaxR; ++i) {
    const int r = wave + i * (NT / 64);
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < kSeMaxC64; ++j) a += w1r[i][j] * mj[j];
    a = pv_wave_sum(a);
    if (lane == 0 && r < 32) s_hid[r] = r < d.cr ? fmaxf(a + b1r[i], 0.f) : 0.f;
  }
  __syncthreads();
  // ---- fc2 + sigmoid ----
  float hid[CRP];
#pragma unroll
  for (int r = 0; r < CRP; ++r) hid[r] = s_hid[r];
#pragma unroll
  for (int i = 0; i < kSeMaxCh; ++i) {
    const int c = tid + i * NT;
    if (c < d.c_p) {
      const float* wrow = s_w2 + (c < d.C ? c : d.C - 1) * se_w2_pitch(d.cr);
      float w2r[CRP];
#pragma unroll
      for (int r = 0; r < CRP; ++r) w2r[r] = wrow[r];
      float a = b2r[i];
#pragma unroll
      for (int r = 0; r < CRP; ++r) a = __builtin_fmaf(r < d.cr ? w2r[r] : 0.f, hid[r], a);   // fused, as `a += w * h` always compiled here
      d.gate[(long)b * d.c_p + c] = c < d.C ? pv_sigmoid(a) : 0.f;
    }
  }
}

}  // namespace

extern "C" int pv_se_gate(const pv_se_gate_desc* d, pv_stream_t stream) {
  if (!d || !d->psum || !d->gate || !d->w1 || !d->w2) return PV_ERR_INVALID;
  if (d->B <= 0 || d->C <= 0 || d->cr <= 0 || d->nblk <= 0 || d->c_p < d->C || d->c_p % 8) return PV_ERR_INVALID;
  const int groups = kThreads / se_cw(d->c_p);
  dim3 grid(d->B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d->C <= 448 && d->cr <= 32 && d->c_p <= kSeMaxCp) {
    // at most (512 + 32 + 512) + (448 * 33 + 32) floats = 63488 bytes: inside the 64 KB a launch gets without opting in
    const size_t lds_f = sizeof(float) * ((size_t)se_w2_lds_off(d->c_p, groups) + (size_t)d->C * se_w2_pitch(d->cr) + 32);
    const int cj = (d->C + 63) / 64;
    if (cj <= 1 && d->cr <= 8) PV_LAUNCH((se_gate_fast_kernel<1, 8>), grid, dim3(se_threads(1, 8)), lds_f, st, *d);
    else if (cj <= 2 && d->cr <= 8) PV_LAUNCH((se_gate_fast_kernel<2, 8>), grid, dim3(se_threads(2, 8)), lds_f, st, *d);
    else if (cj <= 4 && d->cr <= 16) PV_LAUNCH((se_gate_fast_kernel<4, 16>), grid, dim3(se_threads(4, 16)), lds_f, st, *d);
    else PV_LAUNCH((se_gate_fast_kernel<7, 32>), grid, dim3(se_threads(7, 32)), lds_f, st, *d);
  } else {
    const size_t lds = sizeof(float) * ((size_t)d->c_p + d->cr + (size_t)groups * d->c_p);
    PV_LAUNCH(se_gate_kernel, grid, dim3(kThreads), lds, st, *d);
  }
  return pv_launch_status();
}
