// What the attention kernels of pv_attn.hip and pv_attn64.hip have in common: where a workgroup's work item lies, the
// key order of a score accumulator, the lane <-> lane+32 max exchange and the K / V buffer resources.
#pragma once
#include "pv_common.h"

// pv_attn64.hip, called by pv_attention (pv_attn.hip); PV_ERR_UNSUPPORTED = not its case
int pv_attn_w64_try(const pv_attention_desc& d, hipStream_t s);

// key (within a 32-key sub-tile) of accumulator register r of the swapped product S^T = K Q^T, for the lane half hi
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// One work item = one block of query rows of one (batch, head): where it lies, and the rows of its head in Q / K / V / O.
template <typename T, int D> struct AttnItem {
  int b, h, qblk;
  __device__ const T* q(const pv_attention_desc& d) const { return static_cast<const T*>(d.q) + (long)b * d.q_bs + h * D; }
  __device__ const T* k(const pv_attention_desc& d) const { return static_cast<const T*>(d.k) + (long)b * d.k_bs + h * D; }
  __device__ const T* v(const pv_attention_desc& d) const { return static_cast<const T*>(d.v) + (long)b * d.v_bs + h * D; }
  __device__ T* o(const pv_attention_desc& d) const { return static_cast<T*>(d.o) + (long)b * d.o_bs + h * D; }
};

// XCD-aware order: consecutive work items (same batch / head -> same K / V) share an XCD's L2.
// nqb: query blocks per (batch, head); total: work items of the launch (= gridDim.x).
template <typename T, int D> __device__ __forceinline__ AttnItem<T, D> attn_item(const pv_attention_desc& d, int nqb, int total) {
  int w;
  {
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    const int qn = total >> 3, rn = total & 7;
    w = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
  }
  const int bh = w / nqb;
  AttnItem<T, D> it;
  it.qblk = w - bh * nqb;
  it.b = bh / d.heads;
  it.h = bh - it.b * d.heads;
  return it;
}

// max of a lane's value and that of lane ^ 32, as a v_permlane32_swap (VALU) instead of an LDS bpermute
__device__ __forceinline__ float attn_max_swap32(float mx) {
  const unsigned mu = __builtin_bit_cast(unsigned, mx);
  auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
}

// K or V of one (batch, head) as a buffer resource over its Nk rows of D bf16 channels: a key past Nk reads zeros by the
// range check.  The byte count is 32-bit: the launcher routes K / V beyond that to attn_kernel.
template <int D> __device__ __forceinline__ __amdgpu_buffer_rsrc_t attn_kv_rsrc(const bf16_t* p, int Nk, int ld) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p), 0, (int)(((long)(Nk - 1) * ld + D) * 2), 0x00020000);
}
