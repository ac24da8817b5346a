// The pointer table of pv_frame_views on the host, for pv_frames.hip and for the entry points that take it optionally
// (pv_hdr.hip, pv_region.hip, pv_area.hip): its checks, the check of a record's slice of it, and the prologue that tells a
// launch over frame lists from one over whole videos.  (On the device the table is read by rs_item, pv_rs.h.)
#pragma once
#include "pv_rs.h"

// The 16-bit YUV kernels of pv_frame_views (frame_yuv16_kernel, pv_frames16.hip) on a launch that fv_run (pv_frames.hip) has
// validated and sized: g and lds are rs_item_launch's.
int pv_frame_yuv16_launch(const pv_batch_views_desc& d, const RsItemLaunch& g, size_t lds, pv_stream_t stream);

namespace {

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
  // outside their layouts both dtypes are refused before; a 4-byte packed pixel is one aligned dword, as an fp32 element is
  const bool f32 = f.batch.src_dtype == PV_F32 || rs_packed_px(f.batch.src_layout) == 4, u16 = f.batch.src_dtype == PV_U16;
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

// An entry point whose table is optional: with one its records are slices of it (frame lists), without one whole videos.
// A table only half given and a length without a table are PV_ERR_INVALID; then `supported` -- what the entry point carries
// of the source forms, judged before the table is read -- else PV_ERR_UNSUPPORTED; then run(frames, check_src) with the
// check of a record's `src` that goes with the kind, behind the table's own checks.
template <typename Run> inline int fv_with_table(const pv_frame_views_desc& f, const Run& run, bool supported = true) {
  if ((f.frame_ptrs == nullptr) != (f.frame_ptrs_dev == nullptr)) return PV_ERR_INVALID;
  const bool frames = f.frame_ptrs != nullptr;
  if (!frames && f.n_frame_ptrs != 0) return PV_ERR_INVALID;
  if (!supported) return PV_ERR_UNSUPPORTED;
  if (!frames) return run(false, rs_check_video_src(f.batch.src_dtype, f.batch.src_layout));
  if (int e = fv_check_table(f)) return e;
  return run(true, fv_check_src(f));
}

}  // namespace
