// What pv_frames.hip and pv_frames16.hip share: the item of a workgroup of pv_frame_views and the launch of its 16-bit kernels;
// and what pv_frames.hip, pv_hdr.hip and pv_region.hip share: the host checks of the pointer table.
#pragma once
#include "pv_rs.h"

// The 16-bit YUV kernels of pv_frame_views (frame_yuv16_kernel, pv_frames16.hip) on a launch that fv_run (pv_frames.hip) has
// validated and sized: g and lds are rs_item_launch's.
int pv_frame_yuv16_launch(const pv_batch_views_desc& d, const RsItemLaunch& g, size_t lds, pv_stream_t stream);

namespace {

// The item of this workgroup, clamped into range before anything is addressed through it, and the base address of the
// frame its table row selects: the entry is clamped into [0, N-1] of the item's source before the slice is indexed, so a
// malformed table can never read outside the item's slice.
struct FvItem {
  const pv_view_source* __restrict__ S;
  int view;
  uintptr_t frame;
};
__device__ __forceinline__ FvItem fv_item(const pv_batch_views_desc& d, int zi, int t) {
  const pv_view_item* __restrict__ it = d.items_dev + zi;
  FvItem r;
  r.S = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
  r.view = min(max(it->view, 0), d.n_views - 1);
  const int row = min(max(it->row, 0), d.n_rows - 1);
  const int ts = min(max(d.t_index[(long)row * d.t_stride + t], 0), r.S->N - 1);
  // `src` is a generic pointer loaded from memory: read through it the entry would be a per-lane flat load.  The table is
  // global memory that nothing writes while the kernel runs, so it is read as constant memory: one scalar load.
  typedef const uint64_t __attribute__((address_space(4))) * table_ptr;
  r.frame = (uintptr_t) reinterpret_cast<table_ptr>(reinterpret_cast<uintptr_t>(r.S->src))[ts];
  return r;
}

// The pointer table of a pv_frame_views_desc: both copies, a device copy at a multiple of 8, a positive length.
inline int fv_check_table(const pv_frame_views_desc& f) {
  if (!f.frame_ptrs || !f.frame_ptrs_dev || f.n_frame_ptrs <= 0) return PV_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(f.frame_ptrs_dev) % 8) return PV_ERR_INVALID;
  return PV_OK;
}

// check_src (rs_item_launch) of a launch whose records are slices of that table: `src` is a slice [k, k + N) whose entries are
// frames (non-null; fp32: 4-byte aligned; 16-bit samples: even).  What the check needs is captured by value: it runs once
// per record, over every frame of it.
inline auto fv_check_src(const pv_frame_views_desc& f) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(f.frame_ptrs_dev);
  const uint64_t* table = f.frame_ptrs;
  const uint64_t n_table = (uint64_t)f.n_frame_ptrs;
  const bool f32 = f.batch.src_dtype == PV_F32, u16 = f.batch.src_dtype == PV_U16;   // outside their layouts both are refused before
  return [=](const pv_view_source& v) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(v.src);
    if (at < base || (at - base) % 8) return PV_ERR_INVALID;
    const uint64_t k = (at - base) / 8;
    if (k + (uint64_t)v.N > n_table) return PV_ERR_INVALID;
    for (int i = 0; i < v.N; ++i) {
      const uint64_t p = table[k + i];
      if (!p || (f32 && p % 4) || (u16 && !rs_yuv16_even((uintptr_t)p))) return PV_ERR_INVALID;
    }
    return PV_OK;
  };
}

}  // namespace
