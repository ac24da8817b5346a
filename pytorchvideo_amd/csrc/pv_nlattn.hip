// Wide-head attention of the non-local block (gfx950), bf16 in / out, fp32 accumulation:
//   mode 0 (softmax):      o = softmax(scale * theta phi^T) g
//   mode 1 (dot_product):  o = (theta phi^T) g * scale            (scale = 1 / Nk)
// (reference: pytorchvideo/layers/nonlocal_net.py, NonLocal.forward).  One single-head attention over all T*H*W positions
// of a clip whose head is Ci = 64 .. 512 channels wide.  The attention kernels of pv_attn.hip keep a whole head's output
// accumulators in one wave; at Ci = 512 that is 512 fp32 per query row and does not fit.  Here the two products are split
// differently:
//   * a workgroup = 4 waves owns 64 query rows of one clip and walks the keys in tiles of 64.  The K tile and the V tile sit
//     in LDS at full width (Ci = 512: 65 KB + 66 KB), so one workgroup lives on a CU and a wave has all 512 registers.
//   * score product, split by ROWS: wave w keeps its 16-row strip of theta in registers for the whole launch (Ci / 8 VGPRs)
//     and reduces over all of Ci -- v_mfma_f32_16x16x32_bf16, theta as A operand, one ds_read_b128 of a key row as B operand.
//     A row's 64 scores lie in the 16 lanes of one quarter wave, so the row maximum is four cross-lane steps inside the wave
//     and the row sum stays a per-lane partial until the epilogue: no cross-wave reduction.
//   * the wave writes its strip of P (bf16) and, in softmax mode, the rescale factor of each of its rows to LDS.
//   * value product, split by COLUMNS: wave w owns output channels [w Ci/4, (w+1) Ci/4) of all 64 rows (64 x Ci/4 fp32 =
//     Ci / 4 accumulator registers).  It reads the whole P tile (A operand, ds_read_b128) and only its slice of V, through the
//     LDS transpose read (ds_read_b64_tr_b16: a quarter wave reads a [4 keys][16 channels] block and each lane receives one
//     channel's four keys), so V is staged row-major as it comes from memory.
//   * staging: K(t+1) is requested before the score MFMAs of tile t and written behind them (after the barrier that ends
//     the reads of K(t)); V(t+1) is requested before the value MFMAs and written behind them.  One register set serves both.
//     Keys past Nk and rows past Nq are zero-filled by the buffer range check: no bounds branches.
//   * softmax: online over the key tiles in the exp2 domain, row maxima taken on the raw scores (scale > 0), the running
//     maximum advanced only when a row of the strip exceeds it by more than 8 (the deferred rescale of pv_attn.hip); a
//     strip that does not advance tells the value waves so with one flag and they skip the multiply.
//   * epilogue: normalise (mode 0) or scale (mode 1) in fp32, round once, turn the tile through the K buffer, 16-byte stores.
//   * the workgroups of one clip are consecutive slots of one XCD (its L2 serves K and V to all of them).
#include <math.h>
#include "pv_common.h"

namespace {

constexpr int kNlRows = 64;      // query rows per workgroup: 16 per wave in the score product
constexpr int kNlKeys = 64;      // keys per tile
constexpr int kNlThreads = 256;
constexpr int kNlPld = kNlKeys + 8;          // P row stride (elements): 144 B, the 16 rows of a fragment read hit different banks
constexpr float kNlDefer = 8.0f;
constexpr long kNlLdsMax = 160 * 1024;

typedef short nl_s16x4 __attribute__((ext_vector_type(4)));
typedef short nl_s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) nl_s16x4* nl_lds_s16x4_t;

// LDS plan of a workgroup for Ci = 64 NC
template <int NC> struct NlPlan {
  static constexpr int CI = 64 * NC;
  static constexpr int KLD = CI + 8;         // K row stride: 16 B x odd -> conflict-free ds_read_b128 over 16 rows
  static constexpr int VLD = CI + 16;        // V row stride: 32 B x odd -> the 4 rows of a transpose read lie 8 banks apart
  static constexpr int K_BYTES = kNlKeys * KLD * 2, V_BYTES = kNlKeys * VLD * 2, P_BYTES = kNlRows * kNlPld * 2;
  static constexpr int A_BYTES = kNlRows * 4;            // rescale factor per row (mode 0), 1 / l in the epilogue
  static constexpr int TOTAL = K_BYTES + V_BYTES + P_BYTES + A_BYTES + 16;   // + one flag per strip
  static_assert(TOTAL <= kNlLdsMax, "tiles fit the LDS of a CU");
};

// operand of one clip as a buffer resource over its N rows of CI channels: a row past N reads zeros by the range check
template <int CI> __device__ __forceinline__ __amdgpu_buffer_rsrc_t nl_rsrc(const bf16_t* p, int N, int ld) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p), 0, (int)(((long)(N - 1) * ld + CI) * 2), 0x00020000);
}

template <int NC, int MODE>
__global__ __launch_bounds__(kNlThreads) void nl_attn_kernel(const pv_nonlocal_attention_desc d, int nqb, int total) {
  using P = NlPlan<NC>;
  constexpr int CI = P::CI, KLD = P::KLD, VLD = P::VLD;
  constexpr int NKK = CI / 32;               // K steps of the score product
  constexpr int NCH = CI / 8;                // 16-byte chunks of a row
  constexpr int CW = CI / 4;                 // output channels of a wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* const k_s = reinterpret_cast<bf16_t*>(smem);
  bf16_t* const v_s = reinterpret_cast<bf16_t*>(smem + P::K_BYTES);
  bf16_t* const p_s = reinterpret_cast<bf16_t*>(smem + P::K_BYTES + P::V_BYTES);
  float* const a_s = reinterpret_cast<float*>(smem + P::K_BYTES + P::V_BYTES + P::P_BYTES);
  int* const f_s = reinterpret_cast<int*>(a_s + kNlRows);

  // XCD-aware order: the row tiles of one clip (same K / V) are consecutive slots of one XCD
  int item;
  {
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int qn = total >> 3, rn = total & 7;
    item = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
  }
  const int b = item / nqb, qblk = item - b * nqb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, lg = lane >> 4;

  const bf16_t* __restrict__ Q = static_cast<const bf16_t*>(d.q) + (long)b * d.q_bs;
  const bf16_t* __restrict__ K = static_cast<const bf16_t*>(d.k) + (long)b * d.k_bs;
  const bf16_t* __restrict__ V = static_cast<const bf16_t*>(d.v) + (long)b * d.v_bs;
  bf16_t* __restrict__ O = static_cast<bf16_t*>(d.o) + (long)b * d.o_bs;
  const __amdgpu_buffer_rsrc_t rq = nl_rsrc<CI>(Q, d.Nq, d.ldq);
  const __amdgpu_buffer_rsrc_t rk = nl_rsrc<CI>(K, d.Nk, d.ldk);
  const __amdgpu_buffer_rsrc_t rv = nl_rsrc<CI>(V, d.Nk, d.ldv);
  const int ntiles = (d.Nk + kNlKeys - 1) / kNlKeys;

  // ---- theta strip (A operands), resident: lane (ln, lg) holds row ln, channels 32 kk + 8 lg .. + 8; rows past Nq are zeros ----
  bf16x8 qf[NKK];
  {
    const unsigned off = (unsigned)((qblk * kNlRows + wave * 16 + ln) * d.ldq + lg * 8) * 2u;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
      qf[kk] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, (int)(off + (unsigned)kk * 64u), 0, 0));
  }

  // ---- staging: thread = (key tid / 8 and + 32, chunks tid % 8 + 8 i): 8 lanes cover 128 contiguous bytes of a key row.
  //      The tile offset goes into the VGPR offset, which the range check covers: keys past Nk read zeros. ----
  const int s_key = tid >> 3, s_c = tid & 7;
  pv_u32x4 st[2 * NC];
  auto load_tile = [&](__amdgpu_buffer_rsrc_t r, int ld, int t) __attribute__((always_inline)) {
    const unsigned off = (unsigned)((t * kNlKeys + s_key) * ld + s_c * 8) * 2u, half = (unsigned)(32 * ld) * 2u;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < NC; ++i)
        st[h * NC + i] = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off + (unsigned)h * half + (unsigned)i * 128u), 0, 0);
  };
  auto store_tile = [&](bf16_t* dst, int lds_ld) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < NC; ++i)
        *reinterpret_cast<pv_u32x4*>(dst + (s_key + 32 * h) * lds_ld + s_c * 8 + i * 64) = st[h * NC + i];
  };

  f32x4 acc[4][NC];   // [16-row tile][16-channel tile of the wave's slice]: rows 4 lg + i, channel ln
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NC; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];   // of rows 4 lg + i of the wave's strip (l_run: this lane's keys only)
#pragma unroll
  for (int i = 0; i < 4; ++i) { m_run[i] = -INFINITY; l_run[i] = 0.f; }
  const float sc = d.scale * 1.44269504088896340736f;   // softmax in the exp2 domain

  load_tile(rk, d.ldk, 0);
  store_tile(k_s, KLD);
  load_tile(rv, d.ldv, 0);
  store_tile(v_s, VLD);
  __syncthreads();

  // fragment addresses.  V: lane i of a quarter wave supplies row i / 4, channels 4 (i % 4) .. + 4 of the [4 keys][16 channels]
  // block and receives channel i of its four keys; two reads (keys 8 lg .. + 4, + 4 .. + 8) make the B operand of a K step.
  const bf16_t* const k_rd = k_s + ln * KLD + lg * 8;
  const bf16_t* const p_rd = p_s + ln * kNlPld + lg * 8;
  const bf16_t* const v_rd = v_s + (lg * 8 + (ln >> 2)) * VLD + wave * CW + (ln & 3) * 4;
  bf16_t* const p_wr = p_s + (wave * 16 + lg * 4) * kNlPld + ln;
  auto lds_tr = [&](const bf16_t* p) __attribute__((always_inline)) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((nl_lds_s16x4_t)(unsigned long)(unsigned)(unsigned long)p);   // LDS addresses are 32-bit
  };

  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) load_tile(rk, d.ldk, t + 1);

    // ---- scores of the wave's strip: S[16 rows][64 keys], lane holds rows 4 lg + i, key 16 nt + ln ----
    f32x4 s[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(k_rd + nt * 16 * KLD + kk * 32);
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[kk], kf, s[nt], 0, 0, 0);
      }
    if constexpr (MODE == 0) {
      if ((t + 1) * kNlKeys > d.Nk) {   // ragged last tile: keys >= Nk out of the softmax
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          if (t * kNlKeys + nt * 16 + ln >= d.Nk) s[nt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
      float mx[4];
      bool need = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = fmaxf(fmaxf(s[0][i], s[1][i]), fmaxf(s[2][i], s[3][i]));
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        mx[i] = v * sc;               // sc > 0: the maximum commutes with the scaling (every tile has a key < Nk: finite)
        need |= mx[i] > m_run[i] + kNlDefer;
      }
      // deferred rescale: the running maxima of the strip advance only when some row's tile maximum exceeds its own by more
      // than kNlDefer (the first tile always does: m_run = -inf)
      const int adv = __any(need);
      float alpha[4] = {1.f, 1.f, 1.f, 1.f};
      if (adv) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float m_new = fmaxf(m_run[i], mx[i]);
          alpha[i] = __builtin_amdgcn_exp2f(m_run[i] - m_new);
          m_run[i] = m_new;
          l_run[i] *= alpha[i];
        }
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[nt][i], sc, -m_run[i]));
          l_run[i] += p;
          p_wr[i * kNlPld + nt * 16] = (bf16_t)p;
        }
      if (ln == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a_s[wave * 16 + lg * 4 + i] = alpha[i];
      }
      if (lane == 0) f_s[wave] = adv;
    } else {
      // dot_product: P is the raw score; keys past Nk are zero rows of K (and of V): they contribute exactly 0
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) p_wr[i * kNlPld + nt * 16] = (bf16_t)s[nt][i];
    }
    __syncthreads();   // P (and the factors) visible; everybody is done with K(t)
    if (more) {
      store_tile(k_s, KLD);
      load_tile(rv, d.ldv, t + 1);
    }

    // ---- values: O[64 rows][wave's CW channels] += P[64][64 keys] V[64 keys][CW] ----
    if constexpr (MODE == 0) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (__builtin_amdgcn_readfirstlane(f_s[mt])) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float a = a_s[mt * 16 + lg * 4 + i];
#pragma unroll
            for (int nt = 0; nt < NC; ++nt) acc[mt][nt][i] *= a;
          }
        }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 pf[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) pf[mt] = *reinterpret_cast<const bf16x8*>(p_rd + mt * 16 * kNlPld + ks * 32);
#pragma unroll
      for (int nt = 0; nt < NC; ++nt) {
        const nl_s16x4 lo = lds_tr(v_rd + ks * 32 * VLD + nt * 16);
        const nl_s16x4 up = lds_tr(v_rd + (ks * 32 + 4) * VLD + nt * 16);
        const nl_s16x8 both = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
        const bf16x8 vf = __builtin_bit_cast(bf16x8, both);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[mt], vf, acc[mt][nt], 0, 0, 0);
      }
    }
    __syncthreads();   // everybody is done with V(t), P and the factors
    if (more) store_tile(v_s, VLD);
  }

  // ---- epilogue: normalise / scale in fp32, one rounding, the tile turned through the K buffer, 16-byte stores ----
  if constexpr (MODE == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float l = l_run[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) l += __shfl_xor(l, o, 64);
      if (ln == 0) a_s[wave * 16 + lg * 4 + i] = 1.0f / l;   // l >= 1: the key that set the running maximum
    }
    __syncthreads();
  }
  bf16_t* const o_s = k_s;   // [64 rows][KLD]: the last reads of K lie before two barriers
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = mt * 16 + lg * 4 + i;
      const float f = MODE == 0 ? a_s[r] : d.scale;
#pragma unroll
      for (int nt = 0; nt < NC; ++nt) o_s[r * KLD + wave * CW + nt * 16 + ln] = (bf16_t)(acc[mt][nt][i] * f);
    }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kNlRows * NCH / kNlThreads; ++j) {
    const int id = j * kNlThreads + tid;
    const int r = id / NCH, c = id - r * NCH;
    const int row = qblk * kNlRows + r;
    if (row < d.Nq)
      *reinterpret_cast<bf16x8*>(O + (long)row * d.ldo + c * 8) = *reinterpret_cast<const bf16x8*>(o_s + r * KLD + c * 8);
  }
}

// PV_OK when the geometry (pointers aside) is the kernel's
int nl_check(const pv_nonlocal_attention_desc& d) {
  if (d.B <= 0 || d.Ci <= 0 || d.Nq <= 0 || d.Nk <= 0) return PV_ERR_INVALID;
  if (d.mode != 0 && d.mode != 1) return PV_ERR_INVALID;
  if (!(d.scale > 0.f) || isinf(d.scale)) return PV_ERR_INVALID;   // row maxima are taken before scaling
  if (d.reserved != 0) return PV_ERR_INVALID;
  if (d.ldq % 8 || d.ldk % 8 || d.ldv % 8 || d.ldo % 8) return PV_ERR_INVALID;          // 16-byte accesses
  if (d.q_bs % 8 || d.k_bs % 8 || d.v_bs % 8 || d.o_bs % 8) return PV_ERR_INVALID;
  if (d.ldq < d.Ci || d.ldk < d.Ci || d.ldv < d.Ci || d.ldo < d.Ci) return PV_ERR_INVALID;
  if (d.dtype != PV_BF16) return PV_ERR_UNSUPPORTED;
  if (d.Ci % 64 || d.Ci < 64 || d.Ci > 512) return PV_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside a clip, the zero-filled rows of a ragged last tile included
  auto fits = [&](int n, int ld) { return ((long)pv_round_up(n, 64) * ld + d.Ci) * 2 < 0x7fffffffL; };
  if ((long)d.Nq + 64 > 0x7fffffffL || (long)d.Nk + 64 > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  if (!fits(d.Nq, d.ldq) || !fits(d.Nk, d.ldk) || !fits(d.Nk, d.ldv) || !fits(d.Nq, d.ldo)) return PV_ERR_UNSUPPORTED;
  if ((long)d.B * pv_ceil_div(d.Nq, kNlRows) > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  return PV_OK;
}

template <int NC, int MODE> int nl_launch(const pv_nonlocal_attention_desc& d, hipStream_t s) {
  const int nqb = (int)pv_ceil_div(d.Nq, kNlRows), total = d.B * nqb;
  constexpr int lds = NlPlan<NC>::TOTAL;
  if (lds > 64 * 1024)
    PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(nl_attn_kernel<NC, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  pv_note_kernel("nl_attn_kernel");   // (PV_LAUNCH by hand: the macro splits a two-parameter template at its comma)
  hipLaunchKernelGGL((nl_attn_kernel<NC, MODE>), dim3((unsigned)total), dim3(kNlThreads), (size_t)lds, s, d, nqb, total);
  return pv_launch_status();
}

template <int MODE> int nl_dispatch(const pv_nonlocal_attention_desc& d, hipStream_t s) {
  switch (d.Ci / 64) {
    case 1: return nl_launch<1, MODE>(d, s);
    case 2: return nl_launch<2, MODE>(d, s);
    case 3: return nl_launch<3, MODE>(d, s);
    case 4: return nl_launch<4, MODE>(d, s);
    case 5: return nl_launch<5, MODE>(d, s);
    case 6: return nl_launch<6, MODE>(d, s);
    case 7: return nl_launch<7, MODE>(d, s);
    case 8: return nl_launch<8, MODE>(d, s);
    default: return PV_ERR_UNSUPPORTED;
  }
}

}  // namespace

extern "C" int pv_nonlocal_attention_supported(const pv_nonlocal_attention_desc* d) { return d && nl_check(*d) == PV_OK ? 1 : 0; }

extern "C" int pv_nonlocal_attention(const pv_nonlocal_attention_desc* dp, pv_stream_t stream) {
  if (!dp) return PV_ERR_INVALID;
  const pv_nonlocal_attention_desc& d = *dp;
  if (!d.q || !d.k || !d.v || !d.o) return PV_ERR_INVALID;
  if (((uintptr_t)d.q | (uintptr_t)d.k | (uintptr_t)d.v | (uintptr_t)d.o) & 15) return PV_ERR_INVALID;
  const int r = nl_check(d);
  if (r != PV_OK) return r;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return d.mode == 0 ? nl_dispatch<0>(d, s) : nl_dispatch<1>(d, s);
}
