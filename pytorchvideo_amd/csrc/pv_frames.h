// What pv_frames.hip and pv_frames16.hip share: the item of a workgroup of pv_frame_views and the launch of its 16-bit kernels.
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

}  // namespace
