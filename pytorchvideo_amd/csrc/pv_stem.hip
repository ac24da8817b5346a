// First-layer ("stem") convolutions on a 4-channel-padded input: SlowFast's (1,7,7) / (5,7,7)
// stems (models/slowfast.py:55-60 -> models/stem.py:80-107), X3D's 1x3x3 stem conv
// (models/x3d.py:66-88) and MViT's (3,7,7) patch embedding (models/stem.py:295-338).
//
// With Cin = 3 an 8-channel-padded implicit GEMM multiplies 5/8 zeros and decodes a tap per 16-byte
// chunk.  Here the input is NDHWC with the channel dim padded to 4 (8 bytes per voxel), so two
// W-adjacent voxels are one 16-byte chunk and a whole (dt,dh) row of the window -- kw voxels -- is one
// contiguous run of memory: K is enumerated as (dt, dh, voxel pair, voxel-in-pair, channel) and the
// MFMA B operand (lane (n = lane&15, q = lane>>4) holds k = 8q..8q+7 of voxel column n) is exactly
// two 8-byte loads at x[ti+dt][hi+dh][wi0 + 2*pair + {0,1}][0..3], straight from global memory into
// operand registers (no LDS round trip; the overlapping windows of neighbouring outputs hit in L1/L2).
// Image-border taps use buffer addressing: an out-of-range offset reads as zero.
// Weights are packed [cout][kt][kh][kw rounded up to even][4] (zeros in the padding) and stay in LDS
// for the life of the workgroup; the epilogue (folded BN or bias, activation) is in registers.
#include <stdlib.h>
#include "pv_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPairs = 1024;   // K <= 8192
constexpr unsigned kOOB = 0x80000000u;   // buffer addressing: an out-of-range offset loads zero / drops the store
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Rows [row0, row0 + ROWS) of the host-packed [w_rows][K] filter -> LDS [ROWS][Kp + 8] (16 B x odd: conflict-free
// ds_read_b128), zero-filled past K and past the last packed row.
template <int ROWS>
__device__ __forceinline__ void stage_filter_slab(const pv_conv3d_desc& d, bf16_t* w_s, int row0, int w_rows, int K, int Kp) {
  const bf16_t* __restrict__ Wt = static_cast<const bf16_t*>(d.w);
  const int cpr = Kp / 8, WLD = Kp + 8;
  for (int id = threadIdx.x; id < ROWS * cpr; id += kThreads) {
    const int r = id / cpr, kc = id - r * cpr;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row0 + r < w_rows && kc * 8 < K) v = *reinterpret_cast<const bf16x8*>(Wt + (long)(row0 + r) * K + kc * 8);
    *reinterpret_cast<bf16x8*>(w_s + r * WLD + kc * 8) = v;
  }
}

// Tap table of the packed K: voxel pair -> dt | dh << 8 | dw << 16, -1 for the pairs that pad K to a multiple of 32.
__device__ __forceinline__ void fill_tap_table(int* tab_s, int npairs, int PPR, int kt, int kh) {
  for (int pi = threadIdx.x; pi < npairs; pi += kThreads) {
    const int row = pi / PPR, pv = pi - row * PPR;
    const int dt = row / kh, dh = row - dt * kh;
    tab_s[pi] = row < kt * kh ? (dt | (dh << 8) | ((2 * pv) << 16)) : -1;
  }
}

// Folded BN (or bias) of channel c < cout: the identity where the descriptor has none.
__device__ __forceinline__ float bn_scale(const pv_conv3d_desc& d, int c) { return d.scale ? d.scale[c] : 1.f; }
__device__ __forceinline__ float bn_shift(const pv_conv3d_desc& d, int c) { return d.shift ? d.shift[c] : 0.f; }
// ... of the four channels c0 .. c0+3 a lane holds; 0 / 0 for the pad channels past cout
__device__ __forceinline__ void load_bn4(const pv_conv3d_desc& d, int c0, float (&sc)[4], float (&sh)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = c0 + j < d.cout;
    sc[j] = ok ? bn_scale(d, c0 + j) : 0.f;
    sh[j] = ok ? bn_shift(d, c0 + j) : 0.f;
  }
}

// The epilogue of four channels c0 .. c0+3, always in this order: affine -> activation -> [position tables, added by the
// caller] -> zero the pad channels -> round.  The store (fp32 / bf16, plain / buffer) is the caller's.
__device__ __forceinline__ void ep_affine_act(float (&v)[4], const f32x4& acc, const float (&sc)[4], const float (&sh)[4], int act) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = acc[j] * sc[j] + sh[j];
  pv_apply_act_n<true>(v, act);
}
__device__ __forceinline__ void ep_zero_pad(float (&v)[4], int c0, int cout) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j >= cout) v[j] = 0.f;
}
__device__ __forceinline__ bf16x4 ep_round(const float (&v)[4]) { return bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]}; }

// JP = 2 (c4_wpair): an MFMA column is a PAIR of W-adjacent outputs whose filters -- the same taps shifted
// by the stride -- occupy rows [0,8) and [8,16) of one filter tile; for an 8-channel layer (SlowFast's
// fast stem) that doubles the useful rows per instruction and halves the operand loads per output.
template <int NT, int TM, int JP = 1>
__global__ __launch_bounds__(kThreads) void stem_c4_kernel(const pv_conv3d_desc d, int ksteps, int ngroups) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int Kp = ksteps * 32;
  const int WLD = Kp + 8;
  bf16_t* w_s = reinterpret_cast<bf16_t*>(smem_raw);
  int* tab_s = reinterpret_cast<int*>(smem_raw + (size_t)NT * 16 * WLD * 2);   // [ksteps*4] pair -> (dt, dh, dw)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n16 = lane & 15, q = lane >> 4;
  const int kw_eff = d.kw + (JP - 1) * d.sw;   // columns spanned by the JP windows of an MFMA column
  const int KWP = (kw_eff + 1) & ~1;
  const int PPR = KWP / 2;                 // voxel pairs per (dt,dh) row
  const int K = d.kt * d.kh * KWP * 4;     // packed K (multiple of 8)
  const int npairs = ksteps * 4;
  const int Wo2 = (d.Wo + JP - 1) / JP;    // MFMA columns per output row
  const long S_out = (long)d.To * d.Ho * Wo2;
  const long M = (long)d.B * S_out;
  const int n0 = blockIdx.y * NT * 16;
  const int w_rows = JP == 1 ? d.cout : JP * pv_round_up(d.cout, 8);   // filter rows the host packed

  stage_filter_slab<NT * 16>(d, w_s, n0, w_rows, K, Kp);
  fill_tap_table(tab_s, npairs, PPR, d.kt, d.kh);
  __syncthreads();

  // buffer descriptor over the whole input (31-bit byte offsets, checked on the host)
  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(d.x), 0, (int)((unsigned)d.B * (unsigned)d.x_bs * 2u), 0x00020000);

  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long m_base = ((long)g * 4 + wave) * (TM * 16);
    if (m_base >= M) continue;
    int vb[TM], vt[TM], vh[TM], vw[TM], vwo[TM], vpt[TM], vps[TM];
    long vy[TM];
    bool vok[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const long m = m_base + t * 16 + n16;
      vok[t] = m < M;
      const long mm = vok[t] ? m : 0;
      const long b = mm / S_out;
      const long sp = mm - b * S_out;
      const int to = (int)(sp / (d.Ho * Wo2));
      const int r2 = (int)(sp - (long)to * d.Ho * Wo2);
      const int ho = r2 / Wo2;
      const int wo = (r2 - ho * Wo2) * JP;     // first output of the column
      vb[t] = (int)b;
      vt[t] = to * d.st - d.pt;
      vh[t] = ho * d.sh - d.ph;
      vw[t] = wo * d.sw - d.pw;
      vwo[t] = wo;
      vpt[t] = to;
      vps[t] = d.pos_temporal ? ho * d.Wo + wo : (to * d.Ho + ho) * d.Wo + wo;   // row of the spatial / full table
      vy[t] = b * d.y_bs + (((long)to * d.Ho + ho) * d.Wo + wo) * d.ldy;
    }
    auto load_step = [&](u32x2 (&dst)[TM][2], int ks) {
      const int tp = tab_s[ks * 4 + q];
      const int dt = tp & 255, dh = (tp >> 8) & 255, dw = tp >> 16;
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int ti = vt[t] + dt, hi = vh[t] + dh, wi = vw[t] + dw;
        const bool rok = vok[t] && tp >= 0 && (unsigned)ti < (unsigned)d.Ti && (unsigned)hi < (unsigned)d.Hi;
        const unsigned base = (unsigned)vb[t] * (unsigned)d.x_bs + ((unsigned)(ti * d.Hi + hi) * d.Wi + wi) * 4u;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const bool ok = rok && (unsigned)(wi + e) < (unsigned)d.Wi && dw + e < kw_eff;
          dst[t][e] = __builtin_amdgcn_raw_buffer_load_b64(rx, (int)(ok ? (base + 4u * e) * 2u : kOOB), 0, 0);
        }
      }
    };

    f32x4 acc[NT][TM];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int t = 0; t < TM; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x2 xa[TM][2], xb[TM][2];
    auto mma = [&](const u32x2 (&src)[TM][2], int ks) {
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w_s + (a * 16 + n16) * WLD + ks * 32 + q * 8);
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const u32x4 u = {src[t][0][0], src[t][0][1], src[t][1][0], src[t][1][1]};
          acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8, u), acc[a][t], 0, 0, 0);
        }
      }
    };
    load_step(xa, 0);
    for (int ks = 0; ks < ksteps; ks += 2) {
      if (ks + 1 < ksteps) load_step(xb, ks + 1);
      mma(xa, ks);
      if (ks + 1 < ksteps) {
        if (ks + 2 < ksteps) load_step(xa, ks + 2);
        mma(xb, ks + 1);
      }
    }

    if constexpr (JP == 2) {
      // ---- epilogue, paired columns: rows 4q..4q+3 of the tile = channels 4(q&1)..+3 of output j = q>>1 ----
      const int co0 = 4 * (q & 1), j = q >> 1;
      float sc[4], sh[4];
      load_bn4(d, co0, sc, sh);
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (!vok[t] || vwo[t] + j >= d.Wo) continue;
        float v[4];
        ep_affine_act(v, acc[0][t], sc, sh, d.act);
        ep_zero_pad(v, co0, d.cout);
        *reinterpret_cast<bf16x4*>(static_cast<bf16_t*>(d.y) + vy[t] + (long)j * d.ldy + co0) = ep_round(v);
      }
      continue;
    }
    // ---- epilogue: lane holds channels n0 + a*16 + q*4 .. +3 of voxel n16 ----
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int c0 = n0 + a * 16 + q * 4;
      if (c0 >= pv_round_up(d.cout, 8)) continue;   // padding channels up to the 8-multiple are written as zeros
      float sc[4], sh[4];
      load_bn4(d, c0, sc, sh);
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (!vok[t]) continue;
        float v[4];
        ep_affine_act(v, acc[a][t], sc, sh, d.act);
        if (d.pos_spatial != nullptr) {   // position tables of the token stream (fp32 [rows][cout]); wave-uniform branch
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < d.cout) {
              v[j] += d.pos_spatial[(long)vps[t] * d.cout + c0 + j];
              if (d.pos_temporal != nullptr) v[j] += d.pos_temporal[(long)vpt[t] * d.cout + c0 + j];
            }
        }
        ep_zero_pad(v, c0, d.cout);
        if (d.y_f32) *reinterpret_cast<f32x4*>(static_cast<float*>(d.y) + vy[t] + c0) = f32x4{v[0], v[1], v[2], v[3]};
        else *reinterpret_cast<bf16x4*>(static_cast<bf16_t*>(d.y) + vy[t] + c0) = ep_round(v);
      }
    }
  }
}

template <int NT, int TM, int JP = 1> int launch_stem(const pv_conv3d_desc& d, int ksteps, hipStream_t s) {
  const long M = (long)d.B * d.To * d.Ho * ((d.Wo + JP - 1) / JP);
  const long ngroups = pv_ceil_div(M, 4 * TM * 16);
  const int nsplit = JP == 1 ? (int)pv_ceil_div(pv_round_up(d.cout, 8), NT * 16) : 1;
  if (ngroups > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  const size_t lds = (size_t)NT * 16 * (ksteps * 32 + 8) * 2 + (size_t)ksteps * 4 * 4;
  if (lds > 160 * 1024) return PV_ERR_UNSUPPORTED;
  auto kern = stem_c4_kernel<NT, TM, JP>;
  if (lds > 64 * 1024)
    PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long gx = ngroups < 4096 ? ngroups : 4096;
  PV_LAUNCH(kern, dim3((unsigned)gx, (unsigned)nsplit), dim3(kThreads), lds, s, d, ksteps, (int)ngroups);
  pv_note_kernel("stem_c4_kernel");   // (launched through a function pointer: PV_LAUNCH saw only the variable)
  PV_LAUNCH_CHECK();
  return PV_OK;
}


// ---------------------------------------------------------------------------------------
// Halo-tile staging of the two LDS-tiled kernels below.  Thread tid owns voxels i = tid + n * NTHR of the IH x IW input
// tile whose corner is (hi0, wi0) of clip b -- the same voxels in every frame, so the geometry is computed once.  Voxels
// outside the image and whole frames outside the clip (the conv's temporal zero padding) are read at an out-of-range
// offset, i.e. as zeros.
template <int IH, int IW, int NTHR>
struct HaloStage {
  static constexpr int NVOX = IH * IW;
  static constexpr int NLD = (NVOX + NTHR - 1) / NTHR;   // 8-byte loads per thread per frame
  __amdgpu_buffer_rsrc_t rx;
  unsigned frame_bytes, g_off[NLD];
  int Ti;
  __device__ __forceinline__ HaloStage(const pv_conv3d_desc& d, int b, int hi0, int wi0) {
    const bf16_t* X = static_cast<const bf16_t*>(d.x) + (long)b * d.x_bs;
    frame_bytes = (unsigned)(d.Hi * d.Wi) * 8u;
    rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(X), 0, (int)(frame_bytes * (unsigned)d.Ti), 0x00020000);
    Ti = d.Ti;
    const int tid = threadIdx.x;
#pragma unroll
    for (int n = 0; n < NLD; ++n) {
      const int i = tid + n * NTHR;
      const int ir = i / IW, ic = i - ir * IW;
      const int hi = hi0 + ir, wi = wi0 + ic;
      const bool ok = i < NVOX && (unsigned)hi < (unsigned)d.Hi && (unsigned)wi < (unsigned)d.Wi;
      g_off[n] = ok ? (unsigned)(hi * d.Wi + wi) * 8u : kOOB;
    }
  }
  __device__ __forceinline__ void load(int ti, u32x2 (&st)[NLD]) const {
    const bool live = (unsigned)ti < (unsigned)Ti;
#pragma unroll
    for (int n = 0; n < NLD; ++n)
      st[n] = __builtin_amdgcn_raw_buffer_load_b64(rx, (int)((live && g_off[n] != kOOB) ? g_off[n] + (unsigned)ti * frame_bytes : kOOB), 0, 0);
  }
};

// ---------------------------------------------------------------------------------------
// 7 x 7 / stride-2 stems with the input tile in LDS: SlowFast's slow (1,7,7) and fast (5,7,7) stems
// (models/slowfast.py:209-229 -> models/stem.py:80-107).
//
// The kernel above gathers every MFMA B operand straight from global memory: 2.2 KB of window per output voxel of
// the (5,7,7) stem go through L1 / the texture addresser (PMC: 554 MB of HBM traffic against 369 MB algorithmic,
// 18.6 k VALU instructions per wave, most of them address arithmetic) -- 0.79 ms for 99 GFLOP.  Here a workgroup
// owns an 8 x 32 output tile of one clip and walks the T axis:
//   * each input frame's halo tile (21 x 70 voxels x 8 bytes) is staged into LDS ONCE and stays in a ring of kt + 1
//     frames: the 5 temporal taps re-read LDS, not memory; the next frame's loads are in flight during the MFMAs;
//   * with kw = 7 padded to 8, one (dt, dh) row of the window is exactly one K step of 32: lane (n, q) reads ONE
//     aligned 16-byte chunk (voxel pair q of output column n) with a compile-time LDS offset -- no tap table, no
//     bounds tests (the halo is zero-filled at staging time);
//   * the filter is held in LDS as ready-made A fragments (lane-linear 1 KB each: conflict-free ds_read_b128);
//   * <= 8 output channels (fast stem): the 16 MFMA rows are 8 channels x TWO vertically adjacent outputs -- input
//     row r of a row pair feeds output row h with dh = r and output row h+1 with dh = r - 2 -- so no half of the
//     instruction is idle; 64 channels (slow stem): 4 channel tiles share every B fragment.
template <int RP, int NT, int TM, int KT>
__global__ __launch_bounds__(kThreads) void stem7_kernel(const pv_conv3d_desc d, int tiles_h, int tiles_w, int wpitch) {
  constexpr int TH = 8, TW = TM * 16;
  constexpr int IH = (TH - 1) * 2 + 7;       // 21 input rows
  constexpr int IW = (TW - 1) * 2 + 8;       // 70 input columns (even: 16-byte chunks = voxel pairs)
  typedef HaloStage<IH, IW, kThreads> Halo;
  constexpr int NVOX = Halo::NVOX, NLD = Halo::NLD;
  constexpr int FRAME = NVOX * 4;            // bf16 elements per staged frame
  constexpr int JR = RP == 2 ? 9 : 7;        // A fragments per temporal tap (row offsets of a row pair / dh)
  constexpr int NA = RP == 2 ? 1 : NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // KT > 0 (row-pair form only): the temporal extent is a compile-time constant and every wave keeps all KT * 9 A
  // fragments in registers (180 VGPRs for the (5,7,7) stem) -- the LDS then holds nothing but the frame ring
  // (70 KB: two workgroups per CU, one's barrier waits hidden behind the other's MFMAs) and A costs no LDS bandwidth.
  constexpr bool kAReg = RP == 2 && KT > 0;
  bf16_t* wf_s = reinterpret_cast<bf16_t*>(smem_raw);               // [kt][JR][NA][64 lanes][8]
  const int nfrag = kAReg ? 0 : d.kt * JR * NA;
  bf16_t* ring = wf_s + (size_t)nfrag * 512;                         // [kt + 1][IH][IW][4]
  const int nslot = d.kt + 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, q = lane >> 4;
  const int tw = blockIdx.x % tiles_w;
  const int th = (blockIdx.x / tiles_w) % tiles_h;
  const int b = blockIdx.x / (tiles_w * tiles_h);
  const int ho0 = th * TH, wo0 = tw * TW;
  const int hi0 = ho0 * 2 - 3, wi0 = wo0 * 2 - 3;
  const int cout_p8 = pv_round_up(d.cout, 8);

  // ---- filter -> A fragments ----
  {
    const bf16_t* __restrict__ Wt = static_cast<const bf16_t*>(d.w);
    const long Kh = (long)d.kt * 7 * wpitch;     // elements per filter row as the host packed it
    for (int id = tid; id < nfrag * 64; id += kThreads) {
      const int f = id >> 6, l = id & 63;
      const int r = l & 15, qq = l >> 4;
      const int a = f % NA, j = (f / NA) % JR, dt = f / (NA * JR);
      int ch, dh;
      if (RP == 2) { ch = r & 7; dh = j - 2 * (r >> 3); }
      else { ch = a * 16 + r; dh = j; }
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ch < d.cout && dh >= 0 && dh < 7)
        v = *reinterpret_cast<const bf16x8*>(Wt + (long)ch * Kh + (long)(dt * 7 + dh) * wpitch + qq * 8);
      *reinterpret_cast<bf16x8*>(wf_s + (size_t)id * 8) = v;
    }
  }

  const Halo halo(d, b, hi0, wi0);
  u32x2 st[NLD];
  auto load_frame = [&](int ti) { halo.load(ti, st); };
  auto slot_of = [&](int ti) { return (ti + 8 * nslot) % nslot; };
  auto store_frame = [&](int ti) {
    bf16_t* dst = ring + (size_t)slot_of(ti) * FRAME;
#pragma unroll
    for (int n = 0; n < NLD; ++n) {
      const int i = tid + n * kThreads;
      if (i < NVOX) *reinterpret_cast<u32x2*>(dst + (size_t)i * 4) = st[n];
    }
  };

  // ---- epilogue constants ----
  float sc[NA][4], sh[NA][4];
#pragma unroll
  for (int a = 0; a < NA; ++a) load_bn4(d, RP == 2 ? 4 * (q & 1) : a * 16 + 4 * q, sc[a], sh[a]);
  bf16_t* Y = static_cast<bf16_t*>(d.y) + (long)b * d.y_bs;
  const unsigned y_frame_bytes = (unsigned)(d.Ho * d.Wo * d.ldy) * 2u;
  __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(Y, 0, (int)(y_frame_bytes * (unsigned)d.To), 0x00020000);

  // prologue: the first kt frames (all of them in flight at once when kt is a compile-time constant)
  if constexpr (KT > 0) {
    u32x2 pf[KT][NLD];
#pragma unroll
    for (int dt = 0; dt < KT; ++dt) {
      load_frame(dt - d.pt);
#pragma unroll
      for (int n = 0; n < NLD; ++n) pf[dt][n] = st[n];
    }
#pragma unroll
    for (int dt = 0; dt < KT; ++dt) {
#pragma unroll
      for (int n = 0; n < NLD; ++n) st[n] = pf[dt][n];
      store_frame(dt - d.pt);
    }
  } else {
    for (int dt = 0; dt < d.kt; ++dt) {
      load_frame(dt - d.pt);
      store_frame(dt - d.pt);
    }
  }
  bf16x8 areg[kAReg ? KT * JR : 1];
  if constexpr (kAReg) {
    const bf16_t* __restrict__ Wt = static_cast<const bf16_t*>(d.w);
    const long Kh = (long)KT * 7 * wpitch;
    const int ch = n16 & 7;
#pragma unroll
    for (int f = 0; f < KT * JR; ++f) {
      const int j = f % JR, dt = f / JR;
      const int dh = j - 2 * (n16 >> 3);
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ch < d.cout && dh >= 0 && dh < 7)
        v = *reinterpret_cast<const bf16x8*>(Wt + (long)ch * Kh + (long)(dt * 7 + dh) * wpitch + q * 8);
      areg[f] = v;
    }
  }
  __syncthreads();

  for (int to = 0; to < d.To; ++to) {
    const int ti_new = to + 1 - d.pt + d.kt - 1;      // the frame output to+1 needs on top of this one's
    load_frame(to + 1 < d.To ? ti_new : -1);
    if constexpr (RP == 2) {
      f32x4 acc[TM];
#pragma unroll
      for (int t = 0; t < TM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < (KT > 0 ? KT : d.kt); ++dt) {
        const bf16_t* fb = ring + (size_t)slot_of(to - d.pt + dt) * FRAME + ((4 * wave) * IW + 2 * n16 + 2 * q) * 4;
        const bf16_t* wp = wf_s + (size_t)(dt * JR) * 512 + lane * 8;
#pragma unroll
        for (int j = 0; j < JR; ++j) {
          bf16x8 af;
          if constexpr (kAReg) af = areg[dt * JR + j];
          else af = *reinterpret_cast<const bf16x8*>(wp + j * 512);
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const bf16x8 bfv = *reinterpret_cast<const bf16x8*>(fb + (j * IW + 32 * t) * 4);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfv, acc[t], 0, 0, 0);
          }
        }
      }
      store_frame(ti_new);
      // rows 4q..4q+3 of the tile = channels 4(q&1)..+3 of output row 2*wave + (q >> 1)
      const int ho = ho0 + 2 * wave + (q >> 1), co0 = 4 * (q & 1);
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int wo = wo0 + t * 16 + n16;
        float v[4];
        ep_affine_act(v, acc[t], sc[0], sh[0], d.act);
        ep_zero_pad(v, co0, d.cout);
        const bool ok = ho < d.Ho && wo < d.Wo && co0 < cout_p8;
        const unsigned off = ok ? (unsigned)to * y_frame_bytes + (unsigned)((ho * d.Wo + wo) * d.ldy + co0) * 2u : kOOB;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ep_round(v)), ry, (int)off, 0, 0);
      }
    } else {
      f32x4 acc[NT][2][TM];
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
          for (int t = 0; t < TM; ++t) acc[a][rr][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int dt = 0; dt < d.kt; ++dt) {
        const bf16_t* fb = ring + (size_t)slot_of(to - d.pt + dt) * FRAME + (2 * n16 + 2 * q) * 4;
        const bf16_t* wp = wf_s + (size_t)(dt * JR * NT) * 512 + lane * 8;
#pragma unroll
        for (int dh = 0; dh < 7; ++dh) {
          bf16x8 bfv[2][TM];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int t = 0; t < TM; ++t)
              bfv[rr][t] = *reinterpret_cast<const bf16x8*>(fb + ((2 * (wave + 4 * rr) + dh) * IW + 32 * t) * 4);
#pragma unroll
          for (int a = 0; a < NT; ++a) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(wp + (dh * NT + a) * 512);
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
              for (int t = 0; t < TM; ++t)
                acc[a][rr][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfv[rr][t], acc[a][rr][t], 0, 0, 0);
          }
        }
      }
      store_frame(ti_new);
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        const int c0 = a * 16 + 4 * q;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int ho = ho0 + wave + 4 * rr;
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const int wo = wo0 + t * 16 + n16;
            float v[4];
            ep_affine_act(v, acc[a][rr][t], sc[a], sh[a], d.act);
            ep_zero_pad(v, c0, d.cout);
            const bool ok = ho < d.Ho && wo < d.Wo && c0 < cout_p8;
            const unsigned off = ok ? (unsigned)to * y_frame_bytes + (unsigned)((ho * d.Wo + wo) * d.ldy + c0) * 2u : kOOB;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ep_round(v)), ry, (int)off, 0, 0);
          }
        }
      }
    }
    __syncthreads();   // frame ti_new is visible; nobody reads the slot it replaced any more
  }
}

// ---------------------------------------------------------------------------------------
// MViT patch embedding: (kt,7,7) conv, stride (st,4,4), 3 -> 96 channels, fp32 tokens + position tables
// (models/stem.py:289-338, models/vision_transformers.py:357-368).
//
// 96 x 672 filter values are 126 KB as MFMA fragments: with them in LDS no input tile fits beside them twice, and the
// generic kernel above re-gathers every window through L1 (PMC: 736 MB per launch against 257 MB algorithmic).  Here the
// FILTER never enters LDS: wave w owns output channels 16w..16w+15 and streams its kt * 7 A fragments (one per (dt, dh)
// window row: kw = 7 padded to 8 voxels x 4 channels = one K = 32 step) from L2 into registers, one temporal tap ahead; LDS holds only the input halo tile of the kt frames (8 x 16 outputs: 35 x 68 voxels x 8 B per frame),
// staged once and read by every wave -- the B operand of output column n, voxel pair q is ONE aligned 16-byte
// ds_read at a compile-time offset (the halo is zero-filled at staging time: no tap table, no bounds tests).
// 57 KB of LDS and ~170 VGPRs: two workgroups per CU, one loading while the other multiplies.
template <int KT, int NW>
__global__ __launch_bounds__(NW * 64, 3) void stem_pe_kernel(const pv_conv3d_desc d, int tiles_h, int tiles_w, int wpitch) {
  constexpr int TH = 8, TW = 16, S = 4;
  constexpr int IH = (TH - 1) * S + 7;       // 35 input rows
  constexpr int IW = (TW - 1) * S + 8;       // 68 input columns = 34 voxel pairs
  constexpr int HP = IW / 4;                 // 17 even (or odd) pairs per row
  constexpr int NTHR = NW * 64;
  typedef HaloStage<IH, IW, NTHR> Halo;
  constexpr int NVOX = Halo::NVOX, NLD = Halo::NLD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // [KT][IH][even pairs 0..16 | odd pairs 0..16][2 voxels][4]: output column n reads pair 2n + q -- with the pairs of
  // one parity stored contiguously the 16 lanes of a ds_read_b128 phase touch 16 consecutive 16-byte chunks (the
  // natural layout would put lanes n and n + 8 on the same banks: columns are 32 bytes apart)
  bf16_t* tile = reinterpret_cast<bf16_t*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, q = lane >> 4;
  int bid = blockIdx.x;
  const int tw = bid % tiles_w; bid /= tiles_w;
  const int th = bid % tiles_h; bid /= tiles_h;
  const int to = bid % d.To;
  const int b = bid / d.To;
  const int ho0 = th * TH, wo0 = tw * TW;
  const int hi0 = ho0 * S - 3, wi0 = wo0 * S - 3, ti0 = to * d.st - d.pt;

  const Halo halo(d, b, hi0, wi0);
  int l_idx[NLD];   // LDS element index of each staged voxel (the parity permutation above)
#pragma unroll
  for (int n = 0; n < NLD; ++n) {
    const int i = tid + n * NTHR;
    const int ir = i / IW, ic = i - ir * IW;
    const int pr = ic >> 1;
    l_idx[n] = i < NVOX ? ((ir * (IW / 2) + (pr & 1) * HP + (pr >> 1)) * 2 + (ic & 1)) * 4 : -1;
  }
  u32x2 st[2][NLD];   // two frames in flight
  auto load_frame = [&](int fr) { halo.load(ti0 + fr, st[fr & 1]); };
  auto store_frame = [&](int fr) {
#pragma unroll
    for (int n = 0; n < NLD; ++n)
      if (l_idx[n] >= 0) *reinterpret_cast<u32x2*>(tile + (size_t)fr * NVOX * 4 + l_idx[n]) = st[fr & 1][n];
  };

  load_frame(0);
  if (KT > 1) load_frame(1);
  // ---- this wave's filter rows as A fragments, streamed from L2 one temporal tap ahead of their use: every fragment
  //      feeds exactly 8 MFMAs of this workgroup, so nothing is gained by holding all kt * 7 of them (84 VGPRs) ----
  const int ch = wave * 16 + n16;
  const bf16_t* __restrict__ Wt = static_cast<const bf16_t*>(d.w) + (long)(ch < d.cout ? ch : 0) * KT * 7 * wpitch + q * 8;
  bf16x8 areg[2][7];
  auto load_a = [&](int dt, bf16x8 (&a)[7]) {
#pragma unroll
    for (int dh = 0; dh < 7; ++dh) {
      a[dh] = *reinterpret_cast<const bf16x8*>(Wt + (long)(dt * 7 + dh) * wpitch);
      if (ch >= d.cout) a[dh] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  load_a(0, areg[0]);
#pragma unroll
  for (int fr = 0; fr < KT; ++fr) {
    store_frame(fr);
    if (fr + 2 < KT) load_frame(fr + 2);
  }
  __syncthreads();

  // ---- 8 output rows x 16 columns x this wave's 16 channels ----
  f32x4 acc[TH];
#pragma unroll
  for (int r = 0; r < TH; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* bbase = tile + ((q & 1) * HP + n16 + (q >> 1)) * 8;   // pair 2 n16 + q: parity q & 1, index n16 + q / 2
#pragma unroll
  for (int dt = 0; dt < KT; ++dt) {
    if (dt + 1 < KT) load_a(dt + 1, areg[(dt + 1) & 1]);
#pragma unroll
    for (int dh = 0; dh < 7; ++dh) {
      const bf16x8 af = areg[dt & 1][dh];
#pragma unroll
      for (int r = 0; r < TH; ++r) {
        const bf16x8 bfv = *reinterpret_cast<const bf16x8*>(bbase + ((size_t)dt * NVOX + (S * r + dh) * IW) * 4);
        acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfv, acc[r], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // keeps tap dt+2's fragment loads from being hoisted up here (registers)
  }

  // ---- epilogue: lane holds channels 16*wave + 4q .. +3 of column n16 for every row ----
  const int c0 = wave * 16 + 4 * q;
  const int wo = wo0 + n16;
  if (c0 >= pv_round_up(d.cout, 8) || wo >= d.Wo) return;
  float sc[4], sh[4];
  load_bn4(d, c0, sc, sh);
  // every position-table value of the tile is requested BEFORE the first store: the compiler cannot prove that y does
  // not alias the tables and would otherwise wait for each row's loads behind the previous row's store (8 round trips)
  float pos[TH][4];
#pragma unroll
  for (int r = 0; r < TH; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) pos[r][j] = 0.f;
  if (d.pos_spatial != nullptr) {
    float pt[4] = {0.f, 0.f, 0.f, 0.f};
    if (d.pos_temporal != nullptr) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < d.cout) pt[j] = d.pos_temporal[(long)to * d.cout + c0 + j];
    }
#pragma unroll
    for (int r = 0; r < TH; ++r) {
      const int ho = ho0 + r < d.Ho ? ho0 + r : d.Ho - 1;
      const long ps = d.pos_temporal ? (long)ho * d.Wo + wo : ((long)to * d.Ho + ho) * d.Wo + wo;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < d.cout) pos[r][j] = d.pos_spatial[ps * d.cout + c0 + j] + pt[j];
    }
  }
#pragma unroll
  for (int r = 0; r < TH; ++r) {
    const int ho = ho0 + r;
    if (ho >= d.Ho) break;
    float v[4];
    ep_affine_act(v, acc[r], sc, sh, d.act);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += pos[r][j];
    ep_zero_pad(v, c0, d.cout);
    const long yo = (long)b * d.y_bs + (((long)to * d.Ho + ho) * d.Wo + wo) * d.ldy + c0;
    if (d.y_f32) *reinterpret_cast<f32x4*>(static_cast<float*>(d.y) + yo) = f32x4{v[0], v[1], v[2], v[3]};
    else *reinterpret_cast<bf16x4*>(static_cast<bf16_t*>(d.y) + yo) = ep_round(v);
  }
}

// number of waves (16-channel tiles) if the patch-embedding kernel takes this conv, else 0
int stem_pe_waves(const pv_conv3d_desc& d) {
  if (d.dtype != PV_BF16 || d.cin != 4 || d.ldx != 4 || d.dwt_w || d.c4_wpair == 2) return 0;
  if (d.kh != 7 || d.kw != 7 || d.sh != 4 || d.sw != 4 || d.ph != 3 || d.pw != 3) return 0;
  if ((d.kt != 1 && d.kt != 3) || d.pt != d.kt / 2 || d.st < 1) return 0;
  if (d.dil_t > 1 || d.dil_h > 1 || d.dil_w > 1) return 0;
  if ((long)d.Ti * d.Hi * d.Wi * 8 > 0x7fffffffL) return 0;
  const int nw = pv_round_up(d.cout, 16) / 16;
  return (nw == 4 || nw == 6 || nw == 8) ? nw : 0;
}

template <int KT, int NW> int launch_stem_pe(const pv_conv3d_desc& d, int wpitch, hipStream_t s) {
  constexpr int TH = 8, TW = 16;
  const int tiles_h = (d.Ho + TH - 1) / TH, tiles_w = (d.Wo + TW - 1) / TW;
  const size_t lds = (size_t)KT * ((TH - 1) * 4 + 7) * ((TW - 1) * 4 + 8) * 8;
  const long blocks = (long)d.B * d.To * tiles_h * tiles_w;
  if (blocks > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  PV_LAUNCH((stem_pe_kernel<KT, NW>), dim3((unsigned)blocks), dim3(NW * 64), lds, s, d, tiles_h, tiles_w, wpitch);
  PV_LAUNCH_CHECK();
  return PV_OK;
}

// geometry of the LDS-staged 7 x 7 stem kernel: 0 = not this kernel's
int stem7_variant(const pv_conv3d_desc& d) {
  if (d.dtype != PV_BF16 || d.cin != 4 || d.ldx != 4 || d.y_f32 || d.pos_spatial || d.pos_temporal || d.dwt_w) return 0;
  if (d.kh != 7 || d.kw != 7 || d.sh != 2 || d.sw != 2 || d.ph != 3 || d.pw != 3 || d.st != 1) return 0;
  if (d.kt < 1 || d.kt > 7 || d.pt != d.kt / 2 || d.To != d.Ti) return 0;
  if (d.dil_t > 1 || d.dil_h > 1 || d.dil_w > 1) return 0;
  if ((long)d.Ti * d.Hi * d.Wi * 8 > 0x7fffffffL || (long)d.To * d.Ho * d.Wo * d.ldy * 2 > 0x7fffffffL) return 0;
  if (d.cout <= 8) return 2;                                   // row pairs
  if (d.cout % 16 == 0 && d.cout <= 64) return 1;              // channel tiles
  return 0;
}

template <int RP, int NT, int TM, int KT = 0> int launch_stem7(const pv_conv3d_desc& d, int wpitch, hipStream_t s) {
  constexpr int TH = 8, TW = TM * 16;
  constexpr int FRAME_B = ((TH - 1) * 2 + 7) * ((TW - 1) * 2 + 8) * 8;
  const int tiles_h = (d.Ho + TH - 1) / TH, tiles_w = (d.Wo + TW - 1) / TW;
  const int nfrag = (RP == 2 && KT > 0) ? 0 : d.kt * (RP == 2 ? 9 : 7 * NT);
  const size_t lds = (size_t)nfrag * 1024 + (size_t)(d.kt + 1) * FRAME_B;
  if (lds > 160 * 1024) return PV_ERR_UNSUPPORTED;
  auto kern = stem7_kernel<RP, NT, TM, KT>;
  if (lds > 64 * 1024)
    PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long blocks = (long)d.B * tiles_h * tiles_w;
  if (blocks > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  PV_LAUNCH(kern, dim3((unsigned)blocks), dim3(kThreads), lds, s, d, tiles_h, tiles_w, wpitch);
  pv_note_kernel("stem7_kernel");   // (launched through a function pointer: PV_LAUNCH saw only the variable)
  PV_LAUNCH_CHECK();
  return PV_OK;
}

// ---------------------------------------------------------------------------------------
// X3D stem in one pass: conv_xy (1 x kh x kw from the 4-channel input, MFMA) followed, with nothing in
// between (models/x3d.py:66-88: Conv2plus1d(norm=None, activation=None)), by the depthwise temporal
// conv_t (DK x 1 x 1, stride 1, padding DK/2) + folded BN + activation.  A lane owns its voxels for
// the whole clip: it walks the T axis, evaluates one frame of conv_xy per step and scatters it into a
// register ring of DK partial output frames (frame t feeds outputs t-DK/2 .. t+DK/2), so the
// 24-channel intermediate -- 2x the bytes of the RGB input -- never exists in memory and the temporal
// conv needs no halo, no LDS and no second launch.  The ring index is a compile-time constant (the T
// loop is unrolled DK-fold), so "rotating" the ring costs no moves.
template <int V> struct IntC { static constexpr int value = V; };

// Constant e of channel c of the fused temporal stage: e < DK = temporal tap e, e = DK = folded-BN scale, e = DK + 1 =
// shift; 0 for the pad channels past cout.
template <int DK> __device__ __forceinline__ float dwt_const(const pv_conv3d_desc& d, int e, int c) {
  const bool ok = c < d.cout;
  return !ok ? 0.f : e < DK ? d.dwt_w[e * pv_round_up(d.cout, 8) + c] : e == DK ? bn_scale(d, c) : bn_shift(d, c);
}

// Where a lane's outputs go: buffer descriptor over y, byte offsets of its clip, of one frame, and of (voxel i, channel
// 4q) inside a frame (kOOB: no such voxel).
template <int TM> struct DwtOut {
  __amdgpu_buffer_rsrc_t ry;
  unsigned clip, frame, yo[TM];
  __device__ __forceinline__ DwtOut(const pv_conv3d_desc& d, int b) {
    ry = __builtin_amdgcn_make_buffer_rsrc(d.y, 0, (int)((unsigned)d.B * (unsigned)d.y_bs * 2u), 0x00020000);
    clip = (unsigned)b * (unsigned)d.y_bs * 2u;
    frame = (unsigned)(d.Ho * d.Wo * d.ldy) * 2u;
  }
};

// The register ring shared by the two X3D stem kernels below, which differ only in how frame t of conv_xy gets into h.
// `ep(e, a)` returns constant e (dwt_const) of this lane's channels a*16 + 4q .. +3: from registers in one kernel, from
// LDS in the other.  Every method takes R = t mod DK as a type, so every ring index is a compile-time constant.
template <int DK, int NT, int TM, int ACT>
struct DwtRing {
  static constexpr int HALF = DK / 2;
  f32x4 ring[DK][NT][TM];

  __device__ __forceinline__ DwtRing() {
#pragma unroll
    for (int k = 0; k < DK; ++k)
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int i = 0; i < TM; ++i) ring[k][a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // frame t feeds output t + HALF - k with tap k
  template <int R, class Ep>
  __device__ __forceinline__ void scatter(IntC<R>, const f32x4 (&h)[NT][TM], const Ep& ep) {
#pragma unroll
    for (int k = 0; k < DK; ++k) {
      f32x4 (&part)[NT][TM] = ring[(R + HALF - k + DK) % DK];
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int i = 0; i < TM; ++i) part[a][i] += ep(k, a) * h[a][i];
    }
  }

  // output t - HALF is complete after frame t: BN, activation, store; its ring slot is recycled for output t + HALF + 1
  // (also for the "outputs" before the first frame, which only exist as garbage in the ring)
  template <int R, class Ep>
  __device__ __forceinline__ void emit(IntC<R>, const pv_conv3d_desc& d, int t, const DwtOut<TM>& out, const Ep& ep) {
    const int q = (threadIdx.x & 63) >> 4;
    const int to = t - HALF;
    constexpr int slot = (R - HALF + DK) % DK;
    f32x4 (&done)[NT][TM] = ring[slot];
    if (to >= 0 && to < d.To) {
      const unsigned fb = out.clip + (unsigned)to * out.frame;
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        const bool cok = a * 16 + q * 4 < pv_round_up(d.cout, 8);   // padding channels up to the 8-multiple are written as zeros
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          f32x4 v = done[a][i] * ep(DK, a) + ep(DK + 1, a);
          if (ACT == PV_ACT_RELU) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
          }
          const bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
          const unsigned off = cok ? out.yo[i] + a * 32u + fb : kOOB;   // kOOB + anything stays out of range
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), out.ry, (int)off, 0, 0);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int i = 0; i < TM; ++i) done[a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // the walk over T, unrolled DK-fold: step(IntC<t mod DK>, t) for t = 0 .. Ti + HALF - 1 (and up to DK - 1 empty steps)
  template <class Step> static __device__ __forceinline__ void walk(int Ti, const Step& step) {
    for (int t0 = 0; t0 < Ti + HALF; t0 += DK) {
      step(IntC<0>{}, t0);
      step(IntC<1>{}, t0 + 1);
      step(IntC<2>{}, t0 + 2);
      if (DK > 3) {
        step(IntC<3 % DK>{}, t0 + 3);
        step(IntC<4 % DK>{}, t0 + 4);
      }
    }
  }
};

template <int NT, int TM, int KS, int DK, int ACT>
__global__ __launch_bounds__(kThreads) void stem_c4_dwt_kernel(const pv_conv3d_desc d, int groups_per_clip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int Kp = KS * 32;
  constexpr int WLD = Kp + 8;
  bf16_t* w_s = reinterpret_cast<bf16_t*>(smem_raw);
  int* tab_s = reinterpret_cast<int*>(smem_raw + (size_t)NT * 16 * WLD * 2);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n16 = lane & 15, q = lane >> 4;
  const int KWP = (d.kw + 1) & ~1;
  const int PPR = KWP / 2;
  const int K = d.kh * KWP * 4;
  const int S_sp = d.Ho * d.Wo;
  const int b = blockIdx.x / groups_per_clip, g = blockIdx.x - b * groups_per_clip;

  stage_filter_slab<NT * 16>(d, w_s, 0, d.cout, K, Kp);
  fill_tap_table(tab_s, KS * 4, PPR, 1, d.kh);
  __syncthreads();

  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(d.x), 0, (int)((unsigned)d.B * (unsigned)d.x_bs * 2u), 0x00020000);

  // ---- this lane's voxels (fixed for the whole clip) and their load / store offsets inside a frame ----
  unsigned xo[TM][KS][2];   // byte offset of the two 8-byte halves of each k-step's fragment, or kOOB
  DwtOut<TM> out(d, b);
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int sp = ((g * 4 + wave) * TM + t) * 16 + n16;
    const bool vok = sp < S_sp;
    const int ho = sp / d.Wo, wo = sp - ho * d.Wo;
    const int h0 = ho * d.sh - d.ph, w0 = wo * d.sw - d.pw;
    out.yo[t] = vok ? (unsigned)(sp * d.ldy + q * 4) * 2u : kOOB;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int tp = tab_s[ks * 4 + q];
      const int dh = (tp >> 8) & 255, dw = tp >> 16;
      const int hi = h0 + dh, wi = w0 + dw;
      const bool rok = vok && tp >= 0 && (unsigned)hi < (unsigned)d.Hi;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool ok = rok && (unsigned)(wi + e) < (unsigned)d.Wi && dw + e < d.kw;
        xo[t][ks][e] = ok ? (unsigned)((hi * d.Wi + wi + e) * 4) * 2u : kOOB;
      }
    }
  }
  const unsigned x_frame = (unsigned)(d.Hi * d.Wi * 4) * 2u, x_clip = (unsigned)b * (unsigned)d.x_bs * 2u;

  // ---- temporal taps, folded BN scale, shift of channels a*16 + 4q .. +3, in registers: ep_r[e][a], e as in dwt_const
  //      (scale and shift through load_bn4: one bounds test per channel guards both loads) ----
  f32x4 ep_r[DK + 2][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float sc[4], sh[4];
    load_bn4(d, a * 16 + q * 4, sc, sh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ep_r[DK][a][j] = sc[j];
      ep_r[DK + 1][a][j] = sh[j];
#pragma unroll
      for (int k = 0; k < DK; ++k) ep_r[k][a][j] = dwt_const<DK>(d, k, a * 16 + q * 4 + j);
    }
  }
  auto ep = [&](int e, int a) { return ep_r[e][a]; };

  u32x2 xr[TM][KS][2];
  auto load_frame = [&](int t) {
    const unsigned fb = x_clip + (unsigned)t * x_frame;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          xr[i][ks][e] = __builtin_amdgcn_raw_buffer_load_b64(rx, (int)(xo[i][ks][e] + fb), 0, 0);   // kOOB + fb stays out of range
  };

  DwtRing<DK, NT, TM, ACT> ring;
  auto step = [&](auto Rc, int t) {   // Rc: IntC<t mod DK>
    if (t < d.Ti) {
      f32x4 h[NT][TM];
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int i = 0; i < TM; ++i) h[a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w_s + (a * 16 + n16) * WLD + ks * 32 + q * 8);
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const u32x4 u = {xr[i][ks][0][0], xr[i][ks][0][1], xr[i][ks][1][0], xr[i][ks][1][1]};
            h[a][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8, u), h[a][i], 0, 0, 0);
          }
        }
      if (t + 1 < d.Ti) load_frame(t + 1);   // next frame's loads fly under this frame's FMAs and stores
      ring.scatter(Rc, h, ep);
    }
    ring.emit(Rc, d, t, out, ep);
  };

  load_frame(0);
  ring.walk(d.Ti, step);
}

// The ring kernels take the activation as a template constant: launch the RELU or the NONE instantiation (the only two
// pv_stem_dwt_supported admits).
template <class... P, class... A>
int launch_relu_or_none(const char* name, int act, void (*relu)(P...), void (*none)(P...), dim3 grid, size_t lds, hipStream_t s, A... args) {
  auto kern = act == PV_ACT_RELU ? relu : none;
  PV_LAUNCH(kern, grid, dim3(kThreads), lds, s, args...);
  pv_note_kernel(name);   // (launched through a function pointer: PV_LAUNCH saw only the variable)
  PV_LAUNCH_CHECK();
  return PV_OK;
}

template <int NT, int TM, int KS, int DK> int launch_stem_dwt(const pv_conv3d_desc& d, hipStream_t s) {
  const long S_sp = (long)d.Ho * d.Wo;
  const long gpc = pv_ceil_div(S_sp, 4 * TM * 16);
  if (gpc * d.B > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  const size_t lds = (size_t)NT * 16 * (KS * 32 + 8) * 2 + (size_t)KS * 4 * 4;
  return launch_relu_or_none("stem_c4_dwt_kernel", d.act, stem_c4_dwt_kernel<NT, TM, KS, DK, PV_ACT_RELU>,
                             stem_c4_dwt_kernel<NT, TM, KS, DK, PV_ACT_NONE>, dim3((unsigned)(gpc * d.B)), lds, s, d, (int)gpc);
}

// ---------------------------------------------------------------------------------------
// The X3D stem reading the CALLER'S clip (x_src_slot, include/pv_mi355x.h): 1 x 3 x 3 conv_xy, stride (1,2,2),
// padding (0,1,1), + the depthwise temporal conv of the kernel above, with the same MFMA K order, register ring,
// BN and activation -- only the load stage differs.  Without it every forward first ran pv_ingest_ncdhw (NCDHW ->
// the 4-channel layout: 154 MB read + 205 MB written for X3D-M's 32 clips), and the kernel above then re-read those
// 205 MB with one small load in flight per wave.
//
// A workgroup owns an 8 x 16 output tile of one clip (wave w: output rows 2w, 2w+1 = the TM = 2 MFMA column groups)
// and walks the T axis.  Each input frame's halo (17 rows x columns [wi0 - 7, wi0 + 41), where wi0 = 2*wo0 - 1 is the
// first input column of the tile) is staged into LDS in the 4-channel layout, double-buffered: frame t+1's loads are
// issued before frame t's MFMAs.  One staging task = one row x 8 voxels (a 16-byte-aligned chunk of every channel
// plane), written as four 16-byte LDS chunks (channel 3 = 0 when the clip has 3).  The B fragment of lane (n, q) is
// the two voxels at LDS column 7 + 2n + dw, exactly the 16 bytes the kernel above loads -- zeros where it loads zeros
// (image border: zero-filled halo; the 4th window column and the unused pairs of K step 1: masked in registers) -- so
// the output is bit-identical.  The slot is read when the kernel starts, so a captured graph follows the input:
//   0                                 -> the 4-channel buffer `x` (filled by the ingest: uint8 / t_index / ... forms);
//   a 16-byte-aligned clip, Wi % 8 == 0 -> one 16-byte load per channel plane and task;
//   any other clip (2-byte aligned)   -> element loads (correct everywhere, slow; no MI355X workload takes it).
// The kernel waits on one frame's loads per step, so what hides the latency is the number of resident workgroups: the
// temporal taps and BN live in LDS and the launch bounds ask for three workgroups per CU (168 VGPRs; two at 244 VGPRs
// took 199 instead of 168 us for X3D-M's 32 clips).  Two frames in flight per workgroup bought nothing: the output
// stores share vmcnt with the loads and retire out of order with them, so the wait for the older frame is vmcnt(0).
constexpr int kDirTH = 8, kDirTW = 16;          // output tile
constexpr int kDirIH = 2 * kDirTH + 1;          // 17 staged input rows
constexpr int kDirNC = 6;                       // 8-voxel chunks per staged row
constexpr int kDirIW = kDirNC * 8;              // 48 staged columns (41 used)
constexpr int kDirTasks = kDirIH * kDirNC;      // 102 (row, chunk) staging tasks per frame
constexpr int kDirFrame = kDirIH * kDirIW * 4;  // bf16 elements per staged frame
enum { kSrcC4 = 0, kSrcVec = 1, kSrcScalar = 2 };

template <int MODE, int NCH, int DK, int ACT>
__device__ __forceinline__ void stem_dir_body(const pv_conv3d_desc& d, const void* src, const bf16_t* w_s, bf16_t* tiles,
                                              f32x4* ep_s, int b, int ho0, int wo0) {
  constexpr int NT = 2, TM = 2, KS = 2;
  constexpr int WLD = KS * 32 + 8;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n16 = lane & 15, q = lane >> 4;
  const int Cs = d.x_src_c;

  // ---- temporal taps, folded BN scale, shift of channels a*16 + 4q .. +3 in LDS: ep_s[(e * NT + a) * 4 + q]
  //      (56 VGPRs a lane less than in registers: three workgroups per CU instead of two) ----
  for (int id = tid; id < (DK + 2) * NT * 4; id += kThreads) {
    const int qq = id & 3, a = (id >> 2) % NT, e = (id >> 2) / NT;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = dwt_const<DK>(d, e, a * 16 + qq * 4 + j);
    ep_s[id] = v;
  }
  // ---- staging task of this thread: row r, chunk c of the halo (threads spread over the four waves) ----
  const int task = lane * 4 + wave;
  const bool has_task = task < kDirTasks;
  const int r = task / kDirNC, c = task - r * kDirNC;
  const int hi = ho0 * 2 - 1 + r, gc = wo0 * 2 - 8 + c * 8;   // gc: first global column of the chunk (multiple of 8)
  const bool rok = has_task && (unsigned)hi < (unsigned)d.Hi;
  const unsigned plane = (unsigned)(d.Hi * d.Wi);               // elements per channel plane of one frame
  __amdgpu_buffer_rsrc_t rx;
  unsigned t_stride, base;   // element offsets: frame step, and (clip, row, chunk) start
  if constexpr (MODE == kSrcC4) {
    rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.x), 0, (int)((unsigned)d.B * (unsigned)d.x_bs * 2u), 0x00020000);
    t_stride = plane * 4u;
    base = (unsigned)b * (unsigned)d.x_bs + ((unsigned)hi * d.Wi + gc) * 4u;
  } else {
    rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(src), 0,
                                           (int)((unsigned)d.B * (unsigned)Cs * (unsigned)d.Ti * plane * 2u), 0x00020000);
    t_stride = plane;
    base = (unsigned)b * (unsigned)Cs * (unsigned)d.Ti * plane + (unsigned)hi * d.Wi + gc;
  }
  // raw loads of one task: C4 = 8 voxels x 8 bytes; Vec / Scalar = 8 elements of each of the 4 channel planes
  u32x4 rw[4];
  auto load_frame = [&](int t) {
    if constexpr (MODE == kSrcC4) {
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        u32x2 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const bool ok = rok && (unsigned)(gc + e + k) < (unsigned)d.Wi;
          v[k] = __builtin_amdgcn_raw_buffer_load_b64(rx, (int)(ok ? (base + (unsigned)t * t_stride + (e + k) * 4u) * 2u : kOOB), 0, 0);
        }
        rw[e / 2] = u32x4{v[0][0], v[0][1], v[1][0], v[1][1]};
      }
    } else if constexpr (MODE == kSrcVec) {
      // Wi % 8 == 0: a chunk is wholly inside or outside.  No branch around a load (planes beyond Cs read out of
      // range = 0): with a fixed number of loads per frame the compiler waits for exactly the ones it needs, and the
      // prefetch stays in flight across the MFMAs and the ring update
      const bool ok = rok && (unsigned)gc < (unsigned)d.Wi;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        rw[ch] = __builtin_amdgcn_raw_buffer_load_b128(
            rx, (int)(ok && ch < Cs ? (base + ((unsigned)ch * d.Ti + t) * plane) * 2u : kOOB), 0, 0);
    } else {
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        unsigned e16[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool ok = rok && ch < Cs && (unsigned)(gc + e) < (unsigned)d.Wi;
          e16[e] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(
              rx, (int)(ok ? (base + ((unsigned)ch * d.Ti + t) * plane + e) * 2u : kOOB), 0, 0);
        }
        rw[ch] = u32x4{e16[0] | (e16[1] << 16), e16[2] | (e16[3] << 16), e16[4] | (e16[5] << 16), e16[6] | (e16[7] << 16)};
      }
    }
  };
  // -> four 16-byte chunks of the 4-channel layout (two voxels each) at row r, columns 8c .. 8c+7 of the staged frame
  auto store_frame = [&](int buf) {
    if (!has_task) return;
    u32x4* dst = reinterpret_cast<u32x4*>(tiles + (size_t)buf * kDirFrame + (size_t)(r * kDirIW + c * 8) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (MODE == kSrcC4) {
        dst[j] = rw[j];
      } else {
        // plane dword j holds voxels 2j (low half) and 2j+1 (high half)
        const unsigned p0 = rw[0][j], p1 = rw[1][j], p2 = rw[2][j], p3 = NCH == 4 ? rw[3][j] : 0u;
        dst[j] = u32x4{(p0 & 0xffffu) | (p1 << 16), (p2 & 0xffffu) | (p3 << 16),
                       (p0 >> 16) | (p1 & 0xffff0000u), (p2 >> 16) | (p3 & 0xffff0000u)};
      }
    }
  };

  // ---- this lane's B fragments: LDS offset and masks per (row group i, K step) ----
  int boff[TM][KS];
  unsigned mlo[KS], mhi[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int pi = ks * 4 + q;              // voxel pair of the packed K (kw = 3 -> 2 pairs per window row)
    const int dh = pi >> 1, dw = 2 * (pi & 1);
    const bool pok = dh < 3;
    mlo[ks] = pok ? ~0u : 0u;
    mhi[ks] = pok && dw == 0 ? ~0u : 0u;    // voxel dw + 1 == 3 is outside the 3-wide window
#pragma unroll
    for (int i = 0; i < TM; ++i)
      boff[i][ks] = ((2 * (2 * wave + i) + (pok ? dh : 0)) * kDirIW + 7 + 2 * n16 + dw) * 4;
  }
  DwtOut<TM> out(d, b);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int ho = ho0 + 2 * wave + i, wo = wo0 + n16;
    out.yo[i] = (ho < d.Ho && wo < d.Wo) ? (unsigned)((ho * d.Wo + wo) * d.ldy + q * 4) * 2u : kOOB;
  }

  auto ep = [&](int e, int a) { return ep_s[(e * NT + a) * 4 + q]; };

  DwtRing<DK, NT, TM, ACT> ring;
  auto step = [&](auto Rc, int t) {   // Rc: IntC<t mod DK>
    if (t < d.Ti) {
      if (t + 1 < d.Ti) load_frame(t + 1);   // in flight under this frame's MFMAs and ring update
      const bf16_t* fr = tiles + (size_t)(t & 1) * kDirFrame;
      f32x4 h[NT][TM];
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int i = 0; i < TM; ++i) h[a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 bv[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(fr + boff[i][ks]);
          const u32x2 hi2 = *reinterpret_cast<const u32x2*>(fr + boff[i][ks] + 4);
          const u32x4 u = {lo[0] & mlo[ks], lo[1] & mlo[ks], hi2[0] & mhi[ks], hi2[1] & mhi[ks]};
          bv[i] = __builtin_bit_cast(bf16x8, u);
        }
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w_s + (a * 16 + n16) * WLD + ks * 32 + q * 8);
#pragma unroll
          for (int i = 0; i < TM; ++i) h[a][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, bv[i], h[a][i], 0, 0, 0);
        }
      }
      ring.scatter(Rc, h, ep);
    }
    // frame t+1 into the other buffer BEFORE this step's output stores: the wait is then for its loads only, and the
    // stores drain behind the barrier
    if (t + 1 < d.Ti) store_frame((t + 1) & 1);
    ring.emit(Rc, d, t, out, ep);
    if (t + 1 < d.Ti) __syncthreads();   // uniform; frame t+1 staged, nobody reads buffer t & 1 any more
  };

  load_frame(0);
  store_frame(0);
  __syncthreads();
  ring.walk(d.Ti, step);
}

template <int DK, int ACT>
__global__ __launch_bounds__(kThreads, 3) void stem_dir_dwt_kernel(const pv_conv3d_desc d, int tiles_h, int tiles_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int NT = 2, Kp = 64;
  bf16_t* w_s = reinterpret_cast<bf16_t*>(smem_raw);
  bf16_t* tiles = w_s + NT * 16 * (Kp + 8);   // [2][kDirIH][kDirIW][4]
  f32x4* ep_s = reinterpret_cast<f32x4*>(tiles + 2 * kDirFrame);   // [DK + 2][NT][4]
  stage_filter_slab<NT * 16>(d, w_s, 0, d.cout, 3 * 4 * 4, Kp);   // packed [cout][kh = 3][kw 3 -> 4][4]
  // (the weights are visible behind the barrier after the first frame is staged)
  int bid = blockIdx.x;
  const int tw = bid % tiles_w; bid /= tiles_w;
  const int th = bid % tiles_h;
  const int b = bid / tiles_h;
  const void* src = *static_cast<const void* const*>(d.x_src_slot);   // uniform: read once per workgroup
  if (src == nullptr)
    stem_dir_body<kSrcC4, 4, DK, ACT>(d, src, w_s, tiles, ep_s, b, th * kDirTH, tw * kDirTW);
  else if (((uintptr_t)src & 15) == 0 && (d.Wi & 7) == 0)   // RGB: three plane loads per task, channel 3 = 0
    d.x_src_c <= 3 ? stem_dir_body<kSrcVec, 3, DK, ACT>(d, src, w_s, tiles, ep_s, b, th * kDirTH, tw * kDirTW)
                   : stem_dir_body<kSrcVec, 4, DK, ACT>(d, src, w_s, tiles, ep_s, b, th * kDirTH, tw * kDirTW);
  else
    stem_dir_body<kSrcScalar, 4, DK, ACT>(d, src, w_s, tiles, ep_s, b, th * kDirTH, tw * kDirTW);
}

template <int DK> int launch_stem_dir(const pv_conv3d_desc& d, hipStream_t s) {
  const int tiles_h = (d.Ho + kDirTH - 1) / kDirTH, tiles_w = (d.Wo + kDirTW - 1) / kDirTW;
  const long blocks = (long)d.B * tiles_h * tiles_w;
  if (blocks > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  const size_t lds = (size_t)2 * 16 * (64 + 8) * 2 + (size_t)2 * kDirFrame * 2 + (size_t)(DK + 2) * 2 * 4 * 16;
  return launch_relu_or_none("stem_dir_dwt_kernel", d.act, stem_dir_dwt_kernel<DK, PV_ACT_RELU>, stem_dir_dwt_kernel<DK, PV_ACT_NONE>,
                             dim3((unsigned)blocks), lds, s, d, tiles_h, tiles_w);
}

}  // namespace

int pv_stem_dwt_supported(const pv_conv3d_desc& d);

// geometry test for the stem above: X3D's conv_xy (1x3x3, stride (1,2,2), padding (0,1,1)) + temporal conv, reading a
// contiguous bf16 [B][x_src_c][Ti][Hi][Wi] clip whose element offsets fit 31 bits
int pv_stem_ncdhw_supported(const pv_conv3d_desc& d) {
  if (!pv_stem_dwt_supported(d)) return 0;
  if (d.kh != 3 || d.kw != 3 || d.sh != 2 || d.sw != 2 || d.ph != 1 || d.pw != 1) return 0;
  if (d.x_src_c < 1 || d.x_src_c > 4 || d.cout > 32) return 0;
  if ((long)d.B * d.x_src_c * d.Ti * d.Hi * d.Wi * 2 > 0x7fffffffL) return 0;
  if ((long)d.B * d.x_bs * 2 > 0x7fffffffL || (long)d.B * d.y_bs * 2 > 0x7fffffffL) return 0;
  return 1;
}

// geometry test for the fused temporal conv: first-layer 1 x kh x kw conv whose K fits two MFMA steps
// (3x3 taps), at most 32 output channels, 3 or 5 temporal taps
int pv_stem_dwt_supported(const pv_conv3d_desc& d) {
  if (d.dtype != PV_BF16 || d.cin != 4 || d.ldx != 4 || d.y_f32) return 0;
  if (d.kt != 1 || d.st != 1 || d.pt != 0 || d.To != d.Ti) return 0;
  if (d.dwt_k != 3 && d.dwt_k != 5) return 0;
  if (d.act != PV_ACT_NONE && d.act != PV_ACT_RELU) return 0;
  if (d.cout > 32 || d.kh * ((d.kw + 1) & ~1) * 4 > 64 || d.kh > 255 || d.kw > 255) return 0;
  return 1;
}

// pv_conv3d with cin == 4 (see include/pv_mi355x.h): bf16 input with 4 channels per voxel, weights
// packed [cout][kt][kh][round_up(kw,2)][4].
int pv_stem_c4(const pv_conv3d_desc& d, hipStream_t s) {
  if (d.dtype != PV_BF16 || d.cin != 4 || d.ldx != 4) return PV_ERR_UNSUPPORTED;
  if (d.residual || d.a_gate || d.a_act != PV_ACT_NONE) return PV_ERR_UNSUPPORTED;
  if ((long)d.B * d.x_bs > 0x3fffffffL) return PV_ERR_UNSUPPORTED;   // 31-bit byte offsets
  if (d.ldy % 4 || d.y_bs % 4) return PV_ERR_INVALID;
  const int jp = d.c4_wpair == 2 ? 2 : 1;
  if (d.c4_wpair < 0 || d.c4_wpair > 2 || (jp == 2 && (d.cout > 8 || d.y_f32 || d.dwt_w))) return PV_ERR_UNSUPPORTED;
  if ((d.pos_spatial || d.pos_temporal) && (!d.pos_spatial || !d.y_f32 || jp == 2 || d.dwt_w)) return PV_ERR_UNSUPPORTED;
  const int KWP = (d.kw + (jp - 1) * d.sw + 1) & ~1;
  const int K = d.kt * d.kh * KWP * 4;
  const int ksteps = (K + 31) / 32;
  if (d.x_src_slot) {   // X3D stem reading the caller's clip (or `x` when the slot holds 0)
    if (!d.dwt_w || !pv_stem_ncdhw_supported(d)) return PV_ERR_UNSUPPORTED;
    return d.dwt_k == 5 ? launch_stem_dir<5>(d, s) : launch_stem_dir<3>(d, s);
  }
  if (d.dwt_w) {   // fused depthwise temporal conv (X3D stem)
    if (!pv_stem_dwt_supported(d)) return PV_ERR_UNSUPPORTED;
    if ((long)d.B * d.y_bs > 0x3fffffffL) return PV_ERR_UNSUPPORTED;
    return d.dwt_k == 5 ? launch_stem_dwt<2, 2, 2, 5>(d, s) : launch_stem_dwt<2, 2, 2, 3>(d, s);
  }
  if (ksteps * 4 > kMaxPairs || d.kt > 255 || d.kh > 255 || d.kw > 255) return PV_ERR_UNSUPPORTED;
  const int cout_p8 = pv_round_up(d.cout, 8);
  if (const int nw = stem_pe_waves(d)) {   // 7 x 7 / stride 4: filter in registers, tile in LDS
    int r = PV_ERR_UNSUPPORTED;
    switch (d.kt * 10 + nw) {   // kt 1 or 3, 4 / 6 / 8 waves (stem_pe_waves)
      case 14: r = launch_stem_pe<1, 4>(d, KWP * 4, s); break;
      case 16: r = launch_stem_pe<1, 6>(d, KWP * 4, s); break;
      case 18: r = launch_stem_pe<1, 8>(d, KWP * 4, s); break;
      case 34: r = launch_stem_pe<3, 4>(d, KWP * 4, s); break;
      case 36: r = launch_stem_pe<3, 6>(d, KWP * 4, s); break;
      case 38: r = launch_stem_pe<3, 8>(d, KWP * 4, s); break;
    }
    if (r != PV_ERR_UNSUPPORTED) return r;
  }
  if (const int v7 = stem7_variant(d)) {   // 7 x 7 / stride 2: input tiles through LDS
    int r;
    if (v7 == 2 && d.kt == 5) r = launch_stem7<2, 1, 2, 5>(d, KWP * 4, s);   // SlowFast's fast stem
    else if (v7 == 2) r = launch_stem7<2, 1, 2>(d, KWP * 4, s);
    else if (d.cout == 64) r = launch_stem7<1, 4, 2>(d, KWP * 4, s);
    else if (d.cout == 48) r = launch_stem7<1, 3, 2>(d, KWP * 4, s);
    else if (d.cout == 32) r = launch_stem7<1, 2, 2>(d, KWP * 4, s);
    else r = launch_stem7<1, 1, 2>(d, KWP * 4, s);
    if (r != PV_ERR_UNSUPPORTED) return r;
  }
  if (jp == 2) return launch_stem<1, 4, 2>(d, ksteps, s);
  if (cout_p8 <= 16) return launch_stem<1, 4>(d, ksteps, s);
  if (cout_p8 <= 32) return launch_stem<2, 4>(d, ksteps, s);
  if (cout_p8 <= 64) return launch_stem<4, 2>(d, ksteps, s);
  // wider outputs (MViT's 96 patch-embedding channels) split over blockIdx.y: 32 filter rows per workgroup keep
  // the LDS-resident filter slab (K up to 672) small enough for two workgroups per CU
  return launch_stem<2, 2>(d, ksteps, s);
}
