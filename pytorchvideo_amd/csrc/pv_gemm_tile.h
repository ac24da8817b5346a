// What the four MFMA GEMM units behind pv_conv3d share (pv_gemm.hip 128 x 128, pv_gemm8.hip ring, pv_gemm9.hip 256 x 256
// eight phases, pv_gemm9h.hip 128 x 256 and transposed): the small device helpers, the steps of the register epilogue, the
// implicit-GEMM stream pieces of the two eight-phase kernels, and the host-side checks, dispatch and launch.  The main loops, the
// LDS layouts and the routing heuristics stay in the units.  Everything here is force-inlined into the kernels (no relocatable
// device code).  A unit takes a piece where all of its kernels keep their VGPR count, private segment and spill counts with it;
// DESIGN.md 3 and profiles/r25/isa_vs_parent.md say which unit takes which piece and the count that kept the others out.
#pragma once
#include "pv_common.h"

// ---------------------------------------------------------------------------------------------- small device helpers
// out-of-image taps, K / M / N tails and the exhausted DMA stream read this page
static __device__ __attribute__((aligned(16))) unsigned int pv_gemm_zero_page[4] = {0u, 0u, 0u, 0u};

// XCD-aware tile order (bijective for any tile count): work item `it` -> origin of its BM (voxels) x BN (channels) tile.
// Tiles are numbered so that consecutive workgroups (same XCD -> same L2) share the activation rows and walk the weight panels.
// The helpers here that read the kernel's variables are structs of REFERENCES to them, built in the kernel -- what a [&] lambda
// is.  With the same values passed as function arguments the compiler allocates registers differently: 13 more VGPRs in the
// eight-phase kernels for the epilogue's finish step, other SGPR spill counts for the tile order.
template <int BM, int BN>
struct PvTileOrder {
  const int& total_tiles;
  const int& tiles_n;
  __device__ __forceinline__ void operator()(int it, long& m0, int& n0) const {
    const int xcd = it & 7, slot = it >> 3;
    const int qn = total_tiles >> 3, rn = total_tiles & 7;
    const int tile = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
    m0 = (long)(tile / tiles_n) * BM;
    n0 = (tile % tiles_n) * BN;
  }
};

// LDS row rho of a weight tile holds output channel chi(rho): within each 32-row MFMA tile, accumulator register r of
// lane-half hi is MFMA row (r&3) + 8*(r>>2) + 4*hi -> channel 16*hi + r
__device__ __forceinline__ int pv_chi(int rho) {
  return (rho & ~31) + 16 * ((rho >> 2) & 1) + 4 * ((rho >> 3) & 3) + (rho & 3);
}

// source selection with bit masks, not `?:` (the compiler would turn a select between two pointers into two exec-masked
// LDS-DMA instructions): p where ok, else the zero page
__device__ __forceinline__ const bf16_t* pv_pick(bool ok, unsigned long p, unsigned long zaddr) {
  const unsigned long m = 0ul - (unsigned long)ok;
  return reinterpret_cast<const bf16_t*>((p & m) | (zaddr & ~m));
}

// s_waitcnt simm16 on gfx9: vmcnt = bits [3:0] | [15:14]; expcnt [6:4] "no wait"; lgkmcnt [11:8]: pv_vm leaves it at "no wait",
// pv_vml waits for lgkmcnt(0) as well
__host__ __device__ constexpr int pv_vm(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }
__host__ __device__ constexpr int pv_vml(int n) { return pv_vm(n) & ~(15 << 8); }

// ---------------------------------------------------------------------------------------------- epilogue
// A lane owns channels cb..cb+15 of one voxel per 32 x 32 accumulator block; a wave's VT voxel blocks are 32 rows apart.
// (pv_gemm and pv_gemm8 finish their accumulators in loops of their own over the global tables: their notes on the per-tile fixed
// cost and on the order of loads and stores stand there.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pv_epi_rsrc(const pv_conv3d_desc& d, bool y_f32) {
  return __builtin_amdgcn_make_buffer_rsrc(d.y, 0, (int)((unsigned)d.B * (unsigned)d.y_bs * (y_f32 ? 4u : 2u)), 0x00020000);
}

// voxel rows m0 + ROWS wm + 32 v + l31 of the lane -> batch item e_b, voxel inside it e_sp, row < M e_ok.  M < 2^31 (host check):
// 32-bit divisions, an order of magnitude cheaper than the 64-bit sequence
template <int VT, int ROWS, typename S>
struct PvEpiRows {
  const long& m0;
  const int& wm;
  const int& l31;
  bool (&e_ok)[VT];
  const long& M;
  long (&e_b)[VT];
  const S& S_out;
  long (&e_sp)[VT];
  __device__ __forceinline__ void operator()() const {
#pragma unroll
    for (int v = 0; v < VT; ++v) {
      const long m = m0 + wm * ROWS + v * 32 + l31;
      e_ok[v] = m < M;
      const long mm = e_ok[v] ? m : 0;
      e_b[v] = (long)((unsigned)mm / (unsigned)S_out);
      e_sp[v] = mm - e_b[v] * S_out;
    }
  }
};

template <int VT> using pv_epi_res_t = f32x4[VT][2][2];   // [v][h8][half]: 8 channels as 2 x f32x4 (fp32) or 1 x 16 bytes (bf16)

// The epilogue of a wave that owns CT x VT accumulator blocks: channels n0 + WS wn + 32 a + 16 hi ..+15 of voxels m0 + 32 VT wm + 32 v
// + l31, whose rows the kernel has decoded into e_b (batch item), e_sp (voxel inside it) and e_ok (row < M).
template <int VT, int WS>
struct PvEpiLoadRes {
  const pv_conv3d_desc& d;
  const int& n0;
  const int& wn;
  const int& hi;
  const bool (&e_ok)[VT];
  const int& cout_p8;
  const long (&e_b)[VT];
  const long (&e_sp)[VT];
  // residual rows of channel tile a
  __device__ __forceinline__ void operator()(const int a, pv_epi_res_t<VT>& res) const {
    if (d.residual == nullptr) return;
    const int cb = n0 + wn * WS + a * 32 + 16 * hi;
#pragma unroll
    for (int v = 0; v < VT; ++v)
#pragma unroll
      for (int h8 = 0; h8 < 2; ++h8) {
        const bool ok = e_ok[v] && cb + h8 * 8 < cout_p8;
        const long ro = ok ? e_b[v] * d.r_bs + e_sp[v] * d.ldr + cb + h8 * 8 : 0;
        if (d.r_f32) {
          const float* rp = static_cast<const float*>(d.residual) + ro;
          res[v][h8][0] = *reinterpret_cast<const f32x4*>(rp);
          res[v][h8][1] = *reinterpret_cast<const f32x4*>(rp + 4);
        } else {
          res[v][h8][0] = *reinterpret_cast<const f32x4*>(static_cast<const bf16_t*>(d.residual) + ro);
        }
      }
  }
};

// tabs: the tile's scale / shift tables in LDS, [scale 256 f32 | shift 256 f32] as the DMA stream left them (channels past cout
// hold a clamped entry: zeroed with the ragged tile)
template <int CT, int VT, int WS>
struct PvEpiFinish {
  const pv_conv3d_desc& d;
  f32x16 (&acc)[CT][VT];
  const float* const& tabs;
  const int& n0;
  const int& wn;
  const int& hi;
  // finish channel tile a in place: scale pass, then shift pass (one 16-register table live at a time), residual, activation,
  // zeros in the ragged tile's padding.  (The activation chain is pv_apply_act_n<true, 16>'s on the accumulator vectors: that
  // helper takes float arrays and tests the activations in another order, which moves the branches in the ISA.)
  __device__ __forceinline__ void operator()(const int a, const pv_epi_res_t<VT>& res) const {
    const int cl = wn * WS + a * 32 + 16 * hi;   // channel inside the tile
    const int cb = n0 + cl;
    if (d.scale != nullptr) {
      f32x4 sc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) sc[q] = *reinterpret_cast<const f32x4*>(tabs + cl + 4 * q);
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] *= sc[r >> 2][r & 3];
    }
    if (d.shift != nullptr) {
      f32x4 sh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) sh[q] = *reinterpret_cast<const f32x4*>(tabs + 256 + cl + 4 * q);
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] += sh[r >> 2][r & 3];
    }
    if (d.residual != nullptr) {
      if (d.r_f32) {
#pragma unroll
        for (int v = 0; v < VT; ++v)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][v][r] += res[v][r >> 3][(r >> 2) & 1][r & 3];
      } else {
#pragma unroll
        for (int v = 0; v < VT; ++v)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][v][r] += (float)__builtin_bit_cast(bf16x8, res[v][r >> 3][0])[r & 7];
      }
    }
    if (d.act == PV_ACT_RELU) {
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] = fmaxf(acc[a][v][r], 0.f);
    } else if (d.act == PV_ACT_GELU) {
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] = pv_gelu_fast(acc[a][v][r]);
    } else if (d.act == PV_ACT_SWISH) {
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] *= pv_sigmoid(acc[a][v][r]);
    } else if (d.act == PV_ACT_SIGMOID) {
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] = pv_sigmoid(acc[a][v][r]);
    }
    if (cb + 16 > d.cout) {   // ragged last channel tile: the padding up to the 8-multiple is written as zeros
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][v][r] = cb + r < d.cout ? acc[a][v][r] : 0.f;
    }
  }
};

// ... then nothing but stores: CT * VT * (fp32 ? 4 : 2) per lane, whatever is masked (a masked store gets an out-of-range buffer
// offset and is dropped by the hardware: every wave issues the same number, which is what makes the counted waits exact).
// YF: 1 / 0 = fp32 / bf16 output known at compile time, -1 = d.y_f32.
template <int CT, int VT, int WS, int YF>
struct PvEpiStore {
  const int& n0;
  const int& wn;
  const int& hi;
  const long (&e_b)[VT];
  const pv_conv3d_desc& d;
  const long (&e_sp)[VT];
  const bool (&e_ok)[VT];
  const int& cout_p8;
  const f32x16 (&acc)[CT][VT];
  const __amdgpu_buffer_rsrc_t& ry;
  __device__ __forceinline__ void operator()() const {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr unsigned kOOB = 0x80000000u;
#pragma unroll
    for (int a = 0; a < CT; ++a) {
      const int cb = n0 + wn * WS + a * 32 + 16 * hi;
#pragma unroll
      for (int v = 0; v < VT; ++v) {
        const unsigned yo = (unsigned)(e_b[v] * d.y_bs + e_sp[v] * d.ldy + cb);   // elements (< 2^31 bytes: host check)
#pragma unroll
        for (int h8 = 0; h8 < 2; ++h8) {
          const bool ok = e_ok[v] && cb + h8 * 8 < cout_p8;
          const int r0 = h8 * 8;
          if (YF < 0 ? (bool)d.y_f32 : YF != 0) {
            const unsigned off = ok ? (yo + r0) * 4u : kOOB;
            __builtin_amdgcn_raw_buffer_store_b128(
                u32x4{__float_as_uint(acc[a][v][r0 + 0]), __float_as_uint(acc[a][v][r0 + 1]),
                      __float_as_uint(acc[a][v][r0 + 2]), __float_as_uint(acc[a][v][r0 + 3])}, ry, (int)off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(
                u32x4{__float_as_uint(acc[a][v][r0 + 4]), __float_as_uint(acc[a][v][r0 + 5]),
                      __float_as_uint(acc[a][v][r0 + 6]), __float_as_uint(acc[a][v][r0 + 7])}, ry,
                (int)(ok ? off + 16u : kOOB), 0, 0);
          } else {
            bf16x8 ob;
#pragma unroll
            for (int r = 0; r < 8; ++r) ob[r] = (bf16_t)acc[a][v][r0 + r];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ob), ry, (int)(ok ? (yo + r0) * 2u : kOOB), 0, 0);
          }
        }
      }
    }
  }
};

// ------------------------------------------------------------- implicit-GEMM stream of the eight-phase kernels (pv_gemm9 / 9h)
// A K step of 64 lies inside ONE tap (the input width is a multiple of 64), so tap, frame / row / column shift and weight column
// are wave-uniform scalars; a thread keeps, per voxel row of its staging rows, the window origin (element offset in x, negative
// for padding rows) and a 24-bit window mask (bit dt | bit 8 + dh | bit 16 + dw set when that tap lies inside the image).
typedef const __attribute__((address_space(1))) void* pv_gptr_t;
typedef __attribute__((address_space(3))) void* pv_lptr_t;
typedef int pv_i32x4 __attribute__((ext_vector_type(4)));

// voxel row m -> window origin (+ chunk8, the thread's K chunk) and window mask.  (References: see PvTileOrder.)
struct PvWindow {
  const pv_conv3d_desc& d;
  const long& M;
  const int& S_out;
  const int& dil_t;   // dilations, at least 1
  const int& dil_h;
  const int& dil_w;
  const int& chunk8;
  __device__ __forceinline__ void operator()(long m, int& off, unsigned& mask) const {
    m = m < M ? m : M - 1;                              // M tail: a clamped row, never stored
    const unsigned b = (unsigned)m / (unsigned)S_out;
    const unsigned sp = (unsigned)m - b * (unsigned)S_out;
    const unsigned to = sp / (unsigned)(d.Ho * d.Wo);
    const unsigned r2 = sp - to * (unsigned)(d.Ho * d.Wo);
    const unsigned ho = r2 / (unsigned)d.Wo;
    const int t0 = (int)to * d.st - d.pt, h0 = (int)ho * d.sh - d.ph, w0 = (int)(r2 - ho * (unsigned)d.Wo) * d.sw - d.pw;
    off = (int)((long)b * d.x_bs + ((long)(t0 * d.Hi + h0) * d.Wi + w0) * d.ldx) + chunk8;
    unsigned msk = 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (q < d.kt && (unsigned)(t0 + q * dil_t) < (unsigned)d.Ti) msk |= 1u << q;
      if (q < d.kh && (unsigned)(h0 + q * dil_h) < (unsigned)d.Hi) msk |= 1u << (8 + q);
      if (q < d.kw && (unsigned)(w0 + q * dil_w) < (unsigned)d.Wi) msk |= 1u << (16 + q);
    }
    mask = msk;
  }
};

// this thread's geometry words, BYTES per thread in LDS behind geo (each thread reads only what it wrote: no synchronisation).
// The address is rebuilt from the thread index behind an empty asm: as a loop-invariant register it was the one value the
// compiler spilled in pv_gemm9, and its reload -- a scratch load + vmcnt(0) in the loop header -- drained the DMA pipeline every
// K-tile pair.
template <bool PW, unsigned BYTES>
__device__ __forceinline__ pv_i32x4 pv_load_geo(const unsigned char* geo, unsigned byte) {
  if constexpr (PW) {
    return pv_i32x4{0, 0, 0, 0};
  } else {
    unsigned t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return *reinterpret_cast<const pv_i32x4*>(geo + t * BYTES + byte);
  }
}

// Start of the stream's tile at voxel row m0.  Temporal-tap rotation (tap_rot: temporal stride 1, whole tiles inside one frame --
// host check): the tile of output frame t starts its reduction at tap (pt - t) mod kt and wraps, so that in step i EVERY concurrent
// tile reads an input frame with index = i (mod kt): the kt consumers of a frame fetch it at the same moment instead of kt times
// through a 4 MB L2 (SlowFast res4 conv_a: 32 tiles per XCD touch 7.3 MB of frames per tap; PMC fetch 2.95 x the input without this)
template <bool PW>
struct PvTapStart {
  int& iss_c0;
  int& iss_dh;
  int& iss_dw;
  const int& tap_rot;
  const int& S_out;
  const pv_conv3d_desc& d;
  int& iss_dt;
  unsigned& iss_wk;
  __device__ __forceinline__ void operator()(const long& m0) const {
    iss_c0 = iss_dh = iss_dw = 0;
    int rot = 0;
    if constexpr (!PW) {
      if (tap_rot) {
        const unsigned sp = (unsigned)m0 % (unsigned)S_out;
        rot = (d.pt - (int)(sp / (unsigned)(d.Ho * d.Wo))) % d.kt;
        rot = rot < 0 ? rot + d.kt : rot;
      }
    }
    iss_dt = rot;
    iss_wk = (unsigned)(rot * d.kh * d.kw * d.cin) * 2u;
  }
};

// folded BatchNorm / bias tables of the stream's tile -> LDS at tab_lds, one 4-byte DMA per thread: wave w < 4 carries
// scale[64 w .. 64 w + 63] of the tile's 256 channels, w >= 4 the shift (channels past cout read a clamped entry: zeroed in the
// epilogue).  The global round trips of 2 x 64 table loads per thread were a third of the per-tile fixed cost (epilogue reads:
// ds_read).  Extra DMAs inside the counted windows only make the waits stricter (an older unit completes earlier), never weaker.
template <class Order>
struct PvIssueTables {
  const int& wave;
  const pv_conv3d_desc& d;
  const bool& iss_live;
  const Order& tile_origin;
  const int& iss_it;
  const int& lane;
  const int& iss_jt;
  __device__ __forceinline__ void operator()(unsigned char* tab_lds) const {
    const float* tab = wave < 4 ? d.scale : d.shift;
    if (tab != nullptr && iss_live) {
      long m0;
      int n0;
      tile_origin(iss_it, m0, n0);
      int n = n0 + 64 * (wave & 3) + lane;
      n = n < d.cout ? n : d.cout - 1;
      __builtin_amdgcn_global_load_lds((pv_gptr_t)(tab + n), (pv_lptr_t)(tab_lds + (iss_jt & 1) * 2048 + wave * 256), 4, 0, 0);
    }
  }
};

// Next K tile of the DMA stream (all of its position is wave-uniform): the tap walk, and behind a tile's last K tile the next
// work item, its staging rows (geom_of: the unit's own) and its tables (issue_tables).
template <bool PW, class Geom, class Tables>
struct PvTapAdvance {
  int& iss_ku;                // K tile inside the work item
  unsigned& iss_wk;           // byte offset of the stream's K tile inside a weight row
  int& iss_c0;                // channel offset inside the tap
  const pv_conv3d_desc& d;
  int& iss_dw;                // tap coordinates
  int& iss_dh;
  int& iss_dt;
  const int& nk;              // K tiles per output tile
  int& iss_it;                // work item
  int& iss_jt;                // this workgroup's tile count
  bool& iss_live;             // work item < total_tiles (the exhausted stream reads the zero page)
  const int& total_tiles;
  const Geom& geom_of;
  const Tables& issue_tables;
  __device__ __forceinline__ void operator()() const {
    ++iss_ku;
    iss_wk += 128u;
    if constexpr (!PW) {
      iss_c0 += 64;
      if (iss_c0 == d.cin) {
        iss_c0 = 0;
        if (++iss_dw == d.kw) {
          iss_dw = 0;
          if (++iss_dh == d.kh) {
            iss_dh = 0;
            if (++iss_dt == d.kt) { iss_dt = 0; iss_wk = 0u; }   // (a rotated reduction wraps to tap 0 = weight column 0)
          }
        }
      }
    }
    if (iss_ku == nk) {
      iss_ku = 0;
      iss_wk = 0u;
      iss_it += gridDim.x;
      ++iss_jt;
      iss_live = iss_it < total_tiles;
      if (iss_live) geom_of(iss_it);
      issue_tables();
    }
  }
};
// ---------------------------------------------------------------------------------------------- host side
// bf16, no gated / activated / second input operand: what every large-tile unit asks
static inline bool pv_gemm_plain_operands(const pv_conv3d_desc& d) {
  return d.dtype == PV_BF16 && d.a_gate == nullptr && d.a_act == PV_ACT_NONE && d.x2 == nullptr;
}
// 31-bit byte offsets in the store descriptor
static inline bool pv_gemm_store_range_ok(const pv_conv3d_desc& d) { return (long)d.B * d.y_bs * (d.y_f32 ? 4 : 2) <= 0x7fffffffL; }

// Can the eight-phase kernels run the geometry at all?  (pointers are not looked at)  K tiles come k_mult / 64 at a time, at least
// k_min / 64 of them.
static inline bool pv_gemm_stream_geometry_ok(const pv_conv3d_desc& d, long k_mult, long k_min, long& M, long& K) {
  if (!pv_gemm_plain_operands(d)) return false;
  if (d.kt > 8 || d.kh > 8 || d.kw > 8) return false;                                // 8-bit window masks per axis
  // dilated convs (detection backbones' res5) stay on the 128 x 128 kernel, whose dilation path has kernel tests
  // (test_dilated_dense_conv); the window masks here fold dil_* in, but no test forces a dilated descriptor onto these tiles
  if (d.dil_t > 1 || d.dil_h > 1 || d.dil_w > 1) return false;
  K = (long)d.kt * d.kh * d.kw * d.cin;
  M = (long)d.B * d.To * d.Ho * d.Wo;
  if (d.cin % 64 != 0 || K % k_mult != 0 || K < k_min) return false;                 // a K step of 64 inside one tap
  // 31-bit element offsets into x, 32-bit byte offsets into w
  if (M > 0x7fffffffL || (long)d.B * d.x_bs > 0x7fffffffL || ((long)d.cout + 256) * K * 2 > 0xffffffffL ||
      (M + 256) * d.ldx * 2 > 0xffffffffL)
    return false;
  return pv_gemm_store_range_ok(d);
}

// GO(PW, YF32) for the run-time pair (rows, yf32); GO returns
#define PV_GEMM_PW_YF32(rows, yf32, GO)                                   \
  do {                                                                    \
    if (yf32) {                                                           \
      if (rows) { GO(true, true); } else { GO(false, true); }             \
    } else {                                                              \
      if (rows) { GO(true, false); } else { GO(false, false); }           \
    }                                                                     \
  } while (0)

// one persistent workgroup per CU on `total` work items, `lds` bytes of dynamic LDS.  (The kernel is launched through a function
// pointer, so its symbol is noted by name: see PV_LAUNCH.)
template <class... P, class... A>
int pv_gemm_launch_persistent(void (*kern)(P...), const char* name, int threads, size_t lds, long total, hipStream_t s, A... args) {
  PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long resident = 256;   // one workgroup per CU
  dim3 grid((unsigned)(total < resident ? total : resident)), block(threads);
  hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
  pv_note_kernel(name);
  PV_LAUNCH_CHECK();
  return PV_OK;
}
