// Fused pooled attention for MViT, bf16, head dim 96 (gfx950):
//   o = softmax((q*scale) k^T) v [+ q]      (reference: pytorchvideo/layers/attention.py:531-539)
//
// Same mathematics and the same lane-private softmax as attn_pipe_kernel (pv_attn.hip): swapped products
// S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, one query per lane, deferred rescale, exp2 domain.
// What differs is the mapping on the CU:
//   * a workgroup = 4 waves = 128 query rows of one (batch, head), each wave owning one 32-row block; a wave stays
//     inside 256 arithmetic registers and uses no accumulator registers, so two workgroups share a CU, two waves a SIMD:
//     every stall of one wave is covered by the other, one workgroup's prologue / epilogue runs beside the other's loop;
//   * V is staged ROW-major ([4 keys][32 channels] blocks of 256 contiguous bytes) and read with
//     ds_read_b64_tr_b16, the LDS transpose read: no transposing stores, no v_perm;
//   * a tile step is 24 MFMAs in two phases -- S^T(t+1) beside the exponentials of tile t, then PV(t) beside the row
//     maxima of tile t+1 -- with ONE barrier between them; K lives in a 2-slot ring, V in a 3-slot ring, so that
//     fragments of the next phase can be requested before the barrier that ends this one;
//   * staging through registers (T14 of the guide: loads issued two steps before their ds_write).
// A form with 64 query rows per wave on one wave per SIMD and a form with one 8-wave workgroup per CU were measured and
// removed: this one won every round in the model (profiles/r6).
#include <type_traits>
#include "pv_attn.h"

namespace {

constexpr int D = 96;          // head dim
constexpr int KT = 64;         // keys per tile
constexpr int kThreads = 256;
constexpr int kRowsWG = 128;   // query rows per workgroup: 32 per wave

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

// the exponential pipeline's batches (see exp_pipe): the 32 elements per lane and tile over 19 MFMA slices, in pairs
constexpr int kExpSlices = 19;
__host__ __device__ constexpr int exp_bound(int g) { return g <= 0 ? 0 : (g >= kExpSlices ? 32 : 2 * ((g * 16) / kExpSlices)); }

// The S^T MFMAs, written out, with every operand in arithmetic registers ("v"): one "a" constraint anywhere makes hipcc
// split the wave's 256 registers 128 / 128 and spill the arithmetic half.  hipcc's hazard recogniser does not look inside
// inline assembly: the consumers of these results are placed 16+ MFMAs behind the last one in the tile loop, and the
// prologue waits explicitly.
__device__ __forceinline__ void mfma_s_first(f32x16& dst, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(dst) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_s_acc(f32x16& dst, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(dst) : "v"(a), "v"(b));
}

__global__ __launch_bounds__(kThreads, 2) void attn_w64_kernel(const pv_attention_desc d, int nqb, int total) {
  using T = bf16_t;
  constexpr int NE = 32;                          // exponentials per lane and tile
  constexpr int KLD = D + 8;                      // K row stride (elements): 16 B * odd -> conflict-free ds_read_b128
  constexpr int NKS = D / 16, NDB = D / 32;
  constexpr int K_BYTES = KT * KLD * 2, V_BYTES = KT * D * 2;
  constexpr int NKF = 2 * NKS;                    // K fragments per tile (sub, ks)
  constexpr int NVF = 4 * NDB;                    // V fragments per tile (sk, db)
  constexpr int KPRE = 4, KRING = KPRE + 1;       // K fragments requested before their phase / ring depth (256 registers have no room for more)
  constexpr int VPRE = 4, VRING = VPRE + 1;
  constexpr int KLEAD = 2, VLEAD = 4;             // MFMA slices between the last pre-read and the end of its phase
  static_assert(NKF >= KPRE && NVF >= VPRE, "rings assume at least KPRE fragments per tile");
  __shared__ __attribute__((aligned(16))) char smem[2 * K_BYTES + 3 * V_BYTES];
  char* const ksm = smem;
  char* const vsm = smem + 2 * K_BYTES;

  const AttnItem<T, D> it = attn_item<T, D>(d, nqb, total);
  const int qblk = it.qblk;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const T* __restrict__ Q = it.q(d);
  const T* __restrict__ K = it.k(d);
  const T* __restrict__ V = it.v(d);
  T* __restrict__ O = it.o(d);

  const int ntiles = (d.Nk + KT - 1) / KT;
  const float sc = d.scale * 1.44269504088896340736f;   // softmax in the exp2 domain

  // ---- Q fragments (B operands), resident for the whole key loop ----
  const int q_row = qblk * kRowsWG + wave * 32 + l31;
  const bool q_ok = q_row < d.Nq;
  bf16x8 qf[NKS];
  {
    const int r = q_ok ? q_row : d.Nq - 1;   // (rows past the end: a valid row, never stored)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(Q + (long)r * d.ldq + ks * 16 + hi * 8);
  }

  // ---- staging: thread = (key tid/4, 16-byte chunk tid%4 of each 32-channel block); keys past Nk read as zeros
  //      (their scores are masked in the last tile, their P is 0) ----
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const int s_key = tid >> 2, s_cq = tid & 3;
  __amdgpu_buffer_rsrc_t rk = attn_kv_rsrc<D>(K, d.Nk, d.ldk);
  __amdgpu_buffer_rsrc_t rv = attn_kv_rsrc<D>(V, d.Nk, d.ldv);
  // two register sets each (by step parity): a tile is requested TWO steps before its ds_write -- the workgroups of a
  // (batch, head) run in lockstep on one XCD and miss its L2 together, so the latency to cover is HBM's, not the L2's
  // (with one set, loads one step ahead, removing the staging from a timing build saved 15 % of the kernel)
  u32x4 kreg[2][NDB], vreg[2][NDB];
  const int k_st = s_key * (KLD * 2) + s_cq * 16;                                  // + i * 64
  const int v_st = (((s_key >> 4) * 4 + ((s_key >> 2) & 3)) * NDB) * 256 + (s_key & 3) * 64 + s_cq * 16;   // + i * 256
  // (the tile offset goes into the VGPR offset, which the buffer's range check covers -- an SGPR offset is not checked:
  //  keys past Nk read zeros)
  const unsigned k_off0 = (unsigned)(s_key * d.ldk + s_cq * 8) * 2u, v_off0 = (unsigned)(s_key * d.ldv + s_cq * 8) * 2u;
  const unsigned k_tile_b = (unsigned)(KT * d.ldk) * 2u, v_tile_b = (unsigned)(KT * d.ldv) * 2u;
  auto load_from = [&](u32x4 (&dst)[NDB], __amdgpu_buffer_rsrc_t r, unsigned off0, unsigned tile_b, int t) __attribute__((always_inline)) {
    const unsigned off = off0 + (unsigned)t * tile_b;
#pragma unroll
    for (int i = 0; i < NDB; ++i) dst[i] = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off + (unsigned)i * 64u), 0, 0);
  };
  auto load_k = [&](int set, int t) __attribute__((always_inline)) { load_from(kreg[set], rk, k_off0, k_tile_b, t); };
  auto load_v = [&](int set, int t) __attribute__((always_inline)) { load_from(vreg[set], rv, v_off0, v_tile_b, t); };
  auto store_k = [&](int set, int slot, int i) __attribute__((always_inline)) {
    *reinterpret_cast<u32x4*>(ksm + slot * K_BYTES + k_st + i * 64) = kreg[set][i];
  };
  auto store_v = [&](int set, int slot, int i) __attribute__((always_inline)) {
    *reinterpret_cast<u32x4*>(vsm + slot * V_BYTES + v_st + i * 256) = vreg[set][i];
  };

  // ---- fragment reads ----
  // K (A operand of S^T): lane (l31, hi) reads key row sub*32 + l31, channels ks*16 + hi*8 .. +8
  const int k_rd = l31 * (KLD * 2) + hi * 16;
  // V (A operand of O^T, through the transpose read): a 16-lane group reads one [4 keys][16 channels] block, lane i of
  // the group supplying the address of row i/4, channels 4*(i%4)..+4 and receiving column i; the two groups of a half
  // wave take the two channel halves of a 32-channel block, hi selects the key quad (keys 4hi.. and 8+4hi.. of a
  // 16-key slot: the order the score accumulators already hold, see pv_attn.hip)
  const int v_rd = hi * (NDB * 256) + ((lane & 15) >> 2) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  bf16x8 kfr[KRING], vfr[VRING];
  // (the slot's base address is formed once per step and hidden from the compiler, so that every fragment address is
  //  that register + an immediate: otherwise hipcc re-associates slot + constant on the scalar unit and spends one
  //  v_add per read)
  auto lds_base = [&](char* p) __attribute__((always_inline)) {
    unsigned a = (unsigned)(unsigned long)p;   // LDS addresses are 32-bit
    asm volatile("" : "+v"(a));
    return (__attribute__((address_space(3))) char*)(unsigned long)a;
  };
  typedef __attribute__((address_space(3))) char* lds_ptr_t;
  auto read_k = [&](lds_ptr_t kb, int f) __attribute__((always_inline)) {   // f = sub * NKS + ks
    const int sub = f / NKS, ks = f - sub * NKS;
    kfr[f % KRING] = *reinterpret_cast<__attribute__((address_space(3))) const bf16x8*>(kb + sub * 32 * (KLD * 2) + ks * 32);
  };
  auto read_v = [&](lds_ptr_t vb, int f) __attribute__((always_inline)) {   // f = sk * NDB + db
    const int sk = f / NDB, db = f - sk * NDB;
    lds_ptr_t p = vb + ((sk * 4) * NDB + db) * 256;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)p);
    const s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(p + 2 * NDB * 256));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 both = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    vfr[f % VRING] = __builtin_bit_cast(bf16x8, both);
  };

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  float mx_next = -1e30f;                // raw (unscaled) row maximum of the scores the next step consumes
  f32x16 sA[2], sB[2];                   // two score sets [32-key sub-tile], swapped by unrolling the tile loop twice

  // One tile step: softmax + PV of tile t (scores in sc_); MORE: the scores of tile t+1 are produced here, into sn.
  //   phase 1: S^T(t+1) MFMAs | exp2 of tile t, P -> bf16 | first V(t) fragments
  //   barrier  (K(t+3) / V(t+2) written in phase 2 of the previous step become visible; everybody is done with K(t+1))
  //   phase 2: PV(t) MFMAs | rest of the exponentials | row maxima of S(t+1) | K(t+3), V(t+2) regs -> LDS, K(t+5), V(t+4)
  //            requested | first K(t+2) fragments
  auto step = [&](auto more_c, auto par_c, int t, f32x16 (&sc_)[2], f32x16 (&sn)[2]) __attribute__((always_inline)) {
    constexpr bool more = decltype(more_c)::value;
    constexpr int par = decltype(par_c)::value;   // t & 1: the staging register set of this step
    const lds_ptr_t kslot = lds_base(ksm + ((t + 1) & 1) * K_BYTES + k_rd);   // K(t+1)
    const lds_ptr_t vslot = lds_base(vsm + (t % 3) * V_BYTES + v_rd);         // V(t)
    const lds_ptr_t knext = lds_base(ksm + (t & 1) * K_BYTES + k_rd);         // K(t+2)
    if (__builtin_expect((t + 1) * KT > d.Nk, 0)) {   // ragged last tile: keys >= Nk out of the softmax, exact row max
      float mx = -1e30f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if ((t * KT + sub * 32 + crow(r, hi)) >= d.Nk) sc_[sub][r] = -1e30f;
          mx = fmaxf(mx, sc_[sub][r]);
        }
      mx_next = mx;
    }
    // ---- deferred rescale: the running max advances only when some lane's tile max exceeds it by more than kDefer ----
    constexpr float kDefer = 8.0f;
    const float mxs = attn_max_swap32(mx_next * sc);   // sc > 0 (pv_attention checks): max commutes with the scaling
    if (__builtin_expect(__any(mxs > m_run + kDefer), 0)) {   // (cold: the register allocator must not pay for it on the common path)
      const float m_new = fmaxf(m_run, mxs);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
    }
    const float neg_m = -m_run;
    float ps[2] = {0.f, 0.f};
    bf16x8 pb[4];   // [16-key slot]
    // element e of the tile's NE exponentials per lane: slot sk = e / 8, then the 8 values of the fragment
    auto exp_range = [&](int e0, int e1) __attribute__((always_inline)) {
#pragma unroll
      for (int e = e0; e < e1; e += 2) {
        const int sk = e / 8, j = e & 7;
        const int sub = sk >> 1, r = (sk & 1) * 8 + j;
        const float p0 = __builtin_amdgcn_exp2f(fmaf(sc_[sub][r], sc, neg_m));
        const float p1 = __builtin_amdgcn_exp2f(fmaf(sc_[sub][r + 1], sc, neg_m));
        ps[0] += p0;
        ps[1] += p1;
        asm volatile("" : "+v"(ps[0]), "+v"(ps[1]));   // (hipcc otherwise keeps all the values alive and sums them at the end)
        pb[sk][j] = (bf16_t)p0;
        pb[sk][j + 1] = (bf16_t)p1;
      }
    };
    // The same work as a three-stage pipeline over the MFMA slices of a step (g = 0 .. NS1 + NS2 - 1): slice g computes
    // the exponent arguments of batch g, the exponentials of batch g-1 and the sums / conversions of batch g-2 -- no
    // instruction waits for the one before it (fma -> exp -> add back to back stalls twice per element).
    // Batch g = elements [exp_bound(g), exp_bound(g+1)), NE elements over kExpSlices slices;
    // slot sk is complete two slices after its last batch, before PV MFMA NS1 + NDB*sk needs it.
    float xv[NE], pv[NE];
    auto exp_pipe = [&](int g) __attribute__((always_inline)) {
#pragma unroll
      for (int e = exp_bound(g - 2); e < exp_bound(g - 1); e += 2) {
        const int sk = e / 8, j = e & 7;
        ps[0] += pv[e];
        ps[1] += pv[e + 1];
        asm volatile("" : "+v"(ps[0]), "+v"(ps[1]));
        pb[sk][j] = (bf16_t)pv[e];
        pb[sk][j + 1] = (bf16_t)pv[e + 1];
      }
#pragma unroll
      for (int e = exp_bound(g - 1); e < exp_bound(g); ++e) pv[e] = __builtin_amdgcn_exp2f(xv[e]);
#pragma unroll
      for (int e = exp_bound(g); e < exp_bound(g + 1); ++e) {
        const int sk = e / 8, j = e & 7;
        xv[e] = fmaf(sc_[sk >> 1][(sk & 1) * 8 + j], sc, neg_m);
      }
    };
    constexpr int NS1 = more ? NKF : 0;          // MFMAs of phase 1
    constexpr int NS2 = NVF;                     // MFMAs of phase 2
    if constexpr (more) {
#pragma unroll
      for (int f = 0; f < NS1; ++f) {
        const int sub = f / NKS, ks = f - sub * NKS;
        if (f + KPRE < NKF) read_k(kslot, f + KPRE);
        if (ks == 0) mfma_s_first(sn[sub], kfr[f % KRING], qf[ks]);
        else mfma_s_acc(sn[sub], kfr[f % KRING], qf[ks]);
        exp_pipe(f);
        // first fragments of V(t), early enough to have landed when the barrier's lgkmcnt(0) is reached
        if (f >= NS1 - VPRE - VLEAD && f < NS1 - VLEAD) read_v(vslot, f - (NS1 - VPRE - VLEAD));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      exp_range(0, 8);
#pragma unroll
      for (int f = 0; f < VPRE; ++f) read_v(vslot, f);
    }
    __syncthreads();
    {
      constexpr int EB = 8;                      // (last step only: exponentials already done)
      constexpr int NE2 = NE - EB;               // ... still to do, under the PV MFMAs of slots 0 .. 2 (slot sk due at NDB*sk)
      constexpr int ESL = 3 * NDB - 1;           // spread over this many PV MFMAs
      float mxa = -1e30f;
#pragma unroll
      for (int f = 0; f < NS2; ++f) {
        const int sk = f / NDB, db = f - sk * NDB;
        if (f + VPRE < NVF) read_v(vslot, f + VPRE);
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[f % VRING], pb[sk], o[db], 0, 0, 0);
        if constexpr (more) exp_pipe(NS1 + f);
        else if (f < ESL) exp_range(EB + 2 * (f * (NE2 / 2) / ESL), EB + 2 * ((f + 1) * (NE2 / 2) / ESL));
        if constexpr (more) {
          // staging: this thread's K(t+3) / V(t+2) registers (requested two steps ago) into LDS, then the registers go
          // back out for K(t+5) / V(t+4)
          if (f >= 2 && f < 2 + NDB) store_k(par, (t + 1) & 1, f - 2);
          if (f == 2 + NDB) load_k(par, t + 5);
          if (f >= 4 + NDB && f < 4 + 2 * NDB) store_v(par, (t + 2) % 3, f - 4 - NDB);
          if (f == 4 + 2 * NDB) load_v(par, t + 4);
          // row maxima of S(t+1) over the last slots (behind the last batch of the exponential pipeline)
          constexpr int M0 = kExpSlices + 2 - NS1, MC = NS2 - M0;
          static_assert(MC > 0 && 4 + 2 * NDB < NS2, "phase 2 has room for the staging and the maxima");
          if (f >= M0) {
            const int a0 = 2 * ((f - M0) * 16 / MC), a1 = 2 * ((f - M0 + 1) * 16 / MC);   // 32 (sub, r) positions in pairs
#pragma unroll
            for (int a = a0; a < a1; a += 2)   // (written out: hipcc puts a canonicalising v_max in front of fmaxf on every asm result)
              asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mxa) : "v"(sn[a >> 4][a & 15]), "v"(sn[a >> 4][(a & 15) + 1]));
            asm volatile("" : "+v"(mxa));   // (the chain stays in its slice)
          }
          // first fragments of K(t+2) (visible since this step's barrier)
          if (f >= NS2 - KPRE - KLEAD && f < NS2 - KLEAD) read_k(knext, f - (NS2 - KPRE - KLEAD));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      mx_next = mxa;
      asm volatile("" : "+v"(mx_next));
    }
    l_run += ps[0] + ps[1];
  };

  // ---- prologue: tiles 0 and 1 staged, K(2) behind them; the scores of tile 0 the plain way ----
  load_k(0, 0);
  load_v(0, 0);
  load_k(1, 1);
  load_v(1, 1);
#pragma unroll
  for (int i = 0; i < NDB; ++i) { store_k(0, 0, i); store_v(0, 0, i); }
  load_k(0, 2);
  load_v(0, 2);
#pragma unroll
  for (int i = 0; i < NDB; ++i) { store_k(1, 1, i); store_v(1, 1, i); }
  load_k(1, 4);
  load_v(1, 3);
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NKF; ++f) {
    const int sub = f / NKS, ks = f - sub * NKS;
    const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(ksm + k_rd + sub * 32 * (KLD * 2) + ks * 32);
    if (ks == 0) mfma_s_first(sA[sub], kf0, qf[ks]);
    else mfma_s_acc(sA[sub], kf0, qf[ks]);
  }
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7");   // MFMA result -> VALU read (see mfma_s_first)
  {
    float mx = -1e30f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sA[sub][r]);
    mx_next = mx;
    // the running max starts at tile 0's (unless that tile is ragged: the step masks it first), so the first step does
    // not take the rescale block for an O that is still zero
    if (KT <= d.Nk) m_run = attn_max_swap32(mx * sc);
  }
  __syncthreads();                       // everybody has read K(0): its slot takes K(2)
  // entering step 0: set 0 = K(3) | V(2), set 1 = K(4) | V(3)  (step t stores K(t+3), V(t+2) from set t&1)
#pragma unroll
  for (int i = 0; i < NDB; ++i) store_k(0, 0, i);
  load_k(0, 3);
#pragma unroll
  for (int f = 0; f < KPRE; ++f) read_k(lds_base(ksm + K_BYTES + k_rd), f);   // first fragments of K(1)
  {
    using Y = std::integral_constant<bool, true>;
    using N = std::integral_constant<bool, false>;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    int t = 0;
    for (; t + 2 < ntiles; t += 2) {
      step(Y{}, P0{}, t, sA, sB);
      step(Y{}, P1{}, t + 1, sB, sA);
    }
    if (ntiles - t == 2) {
      step(Y{}, P0{}, t, sA, sB);
      step(N{}, P1{}, t + 1, sB, sA);
    } else {
      step(N{}, P0{}, t, sA, sB);
    }
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l (+ q), whole rows at a time ----
  // A lane holds 4 channels of each of 12 (block, group) pieces of ITS query: stored from there, every store of a wave
  // touches 32 rows (and the residual's reads likewise).  Instead each wave turns its fp32 block through the (now free)
  // tile rings: 16-byte LDS writes by (query, channel quad), then 8-channel chunks read back in row order, + q in fp32,
  // ONE rounding, 16-byte global accesses in which 12 consecutive lanes cover a row.
  __syncthreads();                                   // every wave is done with the K / V rings
  constexpr int EPITCH = D * 4 + 16;                 // fp32 row + 16 B: rows 4 banks apart, 16-byte aligned
  static_assert(kRowsWG * EPITCH <= 2 * K_BYTES + 3 * V_BYTES, "epilogue staging fits the rings");
  char* const ebase = smem + wave * (32 * EPITCH);
  constexpr int CH = D / 8;                          // 8-channel chunks per row
  static_assert((32 * CH) % 64 == 0, "whole waves of chunks");
  auto wave_sync = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = {o[db][g * 4 + 0] * inv, o[db][g * 4 + 1] * inv, o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv};
      *reinterpret_cast<f32x4*>(ebase + l31 * EPITCH + (db * 32 + 8 * g + 4 * hi) * 4) = v;
    }
  wave_sync();
  const int row0 = qblk * kRowsWG + wave * 32;
#pragma unroll
  for (int i = 0; i < 32 * CH / 64; ++i) {
    const int id = i * 64 + lane;
    const int r = id / CH, c = id - r * CH;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(ebase + r * EPITCH + c * 32);
    const f32x4 up = *reinterpret_cast<const f32x4*>(ebase + r * EPITCH + c * 32 + 16);
    float v[8] = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    const int row = row0 + r;
    if (row < d.Nq) {
      if (d.residual_q) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(Q + (long)row * d.ldq + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)qv[j];
      }
      bf16x8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[j] = (bf16_t)v[j];
      *reinterpret_cast<bf16x8*>(O + (long)row * d.ldo + c * 8) = ov;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)");
}

}  // namespace

// bf16, head dim 96, K / V inside 32-bit byte offsets: launched here.  Anything else is pv_attn.hip's.
int pv_attn_w64_try(const pv_attention_desc& d, hipStream_t s) {
  if (d.dtype != PV_BF16 || d.head_dim != D) return PV_ERR_UNSUPPORTED;
  const long kv_bytes = ((long)d.Nk * (d.ldk > d.ldv ? d.ldk : d.ldv) + d.head_dim) * 2;   // 32-bit buffer offsets
  if (kv_bytes >= 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  const int nqb = (d.Nq + kRowsWG - 1) / kRowsWG;
  const long total = (long)d.B * d.heads * nqb;
  if (total <= 0 || total > 0x7fffffffL) return PV_ERR_UNSUPPORTED;
  PV_LAUNCH(attn_w64_kernel, dim3((unsigned)total), dim3(kThreads), 0, s, d, nqb, (int)total);
  PV_LAUNCH_CHECK();
  return PV_OK;
}
