// The 16-bit YUV 4:2:0 kernels of pv_frame_views (PV_U16 sources: P010 / yuv420p10le surfaces from a decoder's pool), in a
// translation unit of their own; pv_frames.hip validates the descriptor, sizes the launch and calls pv_frame_yuv16_launch.
#include "pv_frames.h"

namespace {

// CSTEP / FORM / D: as rs_strip_yuv.  frame_yuv_kernel (pv_frames.hip) on two-byte samples: one frame is one surface, the
// record's byte offsets and pitches from the frame's (even) base.
template <int CSTEP, int FORM, typename D>
__global__ __launch_bounds__(kRsThreads) void frame_yuv16_kernel(const pv_batch_views_desc d, const RsItemLaunch g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fy_lds[];
  const int t = blockIdx.y;
  const int zi = blockIdx.z;                       // destination item of this launch
  const RsYuvSrc s = rs_item_yuv<CSTEP>(rs_item<RS_FRAMES>(d, zi, t));
  rs_strip_yuv<CSTEP, FORM, D, unsigned short>(fy_lds, g.R, g.pitch, g.pitch_c, g.c_base, s, rs_dst(d, 3), d.yuv2rgb, zi, t, true);
}

}  // namespace

int pv_frame_yuv16_launch(const pv_batch_views_desc& d, const RsItemLaunch& g, size_t lds, pv_stream_t stream) {
  if (d.c_step == 2) RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), frame_yuv16_kernel, 2);
  else RS_DISPATCH(pv_ceil_div(d.Ho, g.R), lds, (d, g), frame_yuv16_kernel, 1);
  PV_LAUNCH_CHECK();
  return PV_OK;
}
