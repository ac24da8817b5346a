// pv_box_views: the person boxes of a key-frame detection forward, mapped from the pixels of each key frame's SOURCE into the
// view pv_batch_views cut from it, written straight into the RoI head's persistent [capacity][5] box buffer.
//
// The box list of a whole call (every key frame of every video) is uploaded once; a forward holds a window of the call's
// item sequence and a window of its boxes, so one launch per forward replaces the host mapping and the host-to-device copy
// of every forward.  One thread per destination row: a row inside the launch loads its box, finds its item (clamped source
// and view, as rs_item of pv_rs.h clamps them) and reads the geometry from that item's record; a row behind the
// launch -- and a box whose item lies outside the window -- becomes {-1, 0, 0, 0, 0}, which pv_roi_align answers with zeros.
// The arithmetic is clip_boxes_to_image, short_side_scale_with_boxes, crop_boxes, clip_boxes_to_image of the reference in
// fp32, every operation rounded on its own: the rule rs_coord (pv_rs.h) uses for coordinates.  Boxes are finite.  Boxes stay
// pixels of the STORED frame: a record with orient != 0 takes them into its displayed frame first (mirror = the reference's
// `width - boxes - 1`, a quarter turn swaps x and y, the corners are re-ordered), and the scale and the window are the
// displayed frame's.
#include "pv_common.h"

namespace {

constexpr int kBoxThreads = 64;

// One coordinate through the pinned steps behind the orientation; n_out is the window size along its axis.
__device__ __forceinline__ float box_coord(float v, float r, int off, int n_out) {
#pragma clang fp contract(off)
  v = v * r;
  v = v - (float)off;
  return fminf(fmaxf(v, 0.f), (float)(n_out - 1));
}

// clip_boxes_to_image along an axis of n pixels.
__device__ __forceinline__ float box_clip(float v, int n) { return fminf(fmaxf(v, 0.f), (float)(n - 1)); }

// A coordinate mirrored along an axis of stored length n: the reference's two operations, `width - boxes - 1`, in that order.
__device__ __forceinline__ float box_mirror(float v, int n) {
#pragma clang fp contract(off)
  float t = (float)n - v;
  t = t - 1.0f;
  return t;
}

__global__ __launch_bounds__(kBoxThreads) void box_views_kernel(const pv_box_views_desc d) {
  const int i = blockIdx.x * kBoxThreads + threadIdx.x;
  if (i >= d.capacity) return;
  float out[5] = {-1.f, 0.f, 0.f, 0.f, 0.f};
  int number = -1;
  if (i < d.n_launch) {
    number = d.box0 + i;                            // < n_boxes: checked on the host
    const int rel = d.box_item[number] - d.item0;
    if (rel >= 0 && rel < d.n_items) {              // item0 + rel < n_seq: checked on the host
      const pv_view_item* __restrict__ it = d.items_dev + (d.item0 + rel);
      const pv_view_source* __restrict__ V = d.sources_dev + min(max(it->source, 0), d.n_sources - 1);
      const int view = min(max(it->view, 0), d.n_views - 1);
      const int Hs = V->Hs, Ws = V->Ws;
      // selected, not indexed
      const int yoff = view == 0 ? V->y_off[0] : (view == 1 ? V->y_off[1] : V->y_off[2]);
      const int xoff = view == 0 ? V->x_off[0] : (view == 1 ? V->x_off[1] : V->x_off[2]);
      const int orient = V->orient & 7, rot = orient & 3;
      const int Hd = (rot & 1) ? Ws : Hs, Wd = (rot & 1) ? Hs : Ws;          // the displayed frame
      const float r = Wd < Hd ? (float)((double)V->Hn / (double)Hd) : (float)((double)V->Wn / (double)Wd);
      const float* __restrict__ b = d.boxes + (long)number * 4;
      float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];                       // pixels of the STORED frame
      if (d.clip_to_source) x1 = box_clip(x1, Ws), y1 = box_clip(y1, Hs), x2 = box_clip(x2, Ws), y2 = box_clip(y2, Hs);
      if (orient != 0) {                                                      // into the displayed frame (include/pv_mi355x.h)
        float xa = x1, ya = y1, xb = x2, yb = y2;
        if (rot == 1) xa = box_mirror(y1, Hs), ya = x1, xb = box_mirror(y2, Hs), yb = x2;
        else if (rot == 2) xa = box_mirror(x1, Ws), ya = box_mirror(y1, Hs), xb = box_mirror(x2, Ws), yb = box_mirror(y2, Hs);
        else if (rot == 3) xa = y1, ya = box_mirror(x1, Ws), xb = y2, yb = box_mirror(x2, Ws);
        if (orient & 4) xa = box_mirror(xa, Wd), xb = box_mirror(xb, Wd);
        x1 = fminf(xa, xb), x2 = fmaxf(xa, xb), y1 = fminf(ya, yb), y2 = fmaxf(ya, yb);
      }
      out[0] = (float)rel;
      out[1] = box_coord(x1, r, xoff, d.Wo);
      out[2] = box_coord(y1, r, yoff, d.Ho);
      out[3] = box_coord(x2, r, xoff, d.Wo);
      out[4] = box_coord(y2, r, yoff, d.Ho);
    }
  }
  float* __restrict__ row = d.dst + (long)i * 5;
#pragma unroll
  for (int k = 0; k < 5; ++k) row[k] = out[k];
  if (d.dst_box) d.dst_box[i] = number;
}

}  // namespace

extern "C" int pv_box_views(const pv_box_views_desc* dp, pv_stream_t stream) {
  if (!dp) return PV_ERR_INVALID;
  const pv_box_views_desc& d = *dp;
  if (!d.boxes || !d.box_item || !d.sources_dev || !d.items_dev || !d.dst) return PV_ERR_INVALID;
  if (d.capacity <= 0 || d.n_items <= 0 || d.Ho <= 0 || d.Wo <= 0 || d.n_sources <= 0) return PV_ERR_INVALID;
  if (d.n_views < 1 || d.n_views > 3) return PV_ERR_INVALID;
  if (d.n_launch < 0 || d.n_launch > d.capacity) return PV_ERR_INVALID;
  if (d.box0 < 0 || d.n_boxes < 0 || (long)d.box0 + d.n_launch > d.n_boxes) return PV_ERR_INVALID;
  if (d.item0 < 0 || d.n_seq <= 0 || (long)d.item0 + d.n_items > d.n_seq) return PV_ERR_INVALID;
  const dim3 grid((unsigned)((d.capacity + kBoxThreads - 1) / kBoxThreads)), block(kBoxThreads);
  PV_LAUNCH(box_views_kernel, grid, block, 0, static_cast<hipStream_t>(stream), d);
  PV_LAUNCH_CHECK();
  return PV_OK;
}
