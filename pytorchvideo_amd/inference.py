"""Whole-video inference: from one decoded video resident on the GPU to its scores, the reference's test protocol end to
end -- `LabeledVideoDataset` + clip sampler (data/clip_sampling.py), `FrameVideo.get_clip` (data/frame_video.py:149-200),
`UniformTemporalSubsample`, `ShortSideScale`, the three `uniform_crop`s, `Div255` + `Normalize`, the forward, and the
per-video fold of pytorchvideo_trainer/module/video_classification.py:244-311.

Nothing is materialised between the video and the first convolution: the sampler's clips become a table of frame numbers
on the host (`data.clip_frame_table`), the table is uploaded once, and the ingest kernel (`pv_video_views`) reads the video
through it, one launch per pathway per forward.  The clips x views sequence is walked in chunks of the deploy form's batch;
the last chunk may be short, so a video of any length runs on a form converted for any batch.
"""
import torch

from .data.clip_sampling import clip_frame_table
from .ensemble import VideoEnsembler
from .transforms import DevicePacker


class VideoPredictor:
    """`VideoPredictor(deployed, clip_sampler, mean, std, div255, short_side, crop_size)(video, fps)` = [num_classes] fp32
    scores of the video: softmax of every view of every clip, summed (`method="sum"`) or maxed ("max") and divided by the
    number of views, as the reference does.  `return_clip_scores=True` adds [n_clips, num_classes]: the same fold over each
    clip's own views (what `UniformClipSampler`'s stride is for on a long video).

    `deployed` is a classification model converted as a whole by `convert_to_deployable_form` (one plan or split-batch);
    `frame_ratios` as for `DevicePacker`; `video` is the decoder's uint8 [N,H,W,3] (`src_layout="NTHWC"`) or a uint8 / fp32
    [C,N,H,W] ("NCTHW") -- or decoder-native YUV 4:2:0, uint8 [N, Hc*3/2, W] with `src_layout` "NV12" / "NV21" / "I420" /
    "YV12" (`yuv`, `coded_height`, `height` as for `DevicePacker`), read in place with the strides it has and converted by
    the ingest itself.  The frame table is built, range-checked and uploaded on EVERY call (one video per call); to score
    the same video again without that, keep `packer.video_tables(...)` and drive `packer.fill_video` / `launch` directly.
    After a call `video_ensembler.counts` (and `clip_ensembler.counts`) hold the rows folded."""

    def __init__(self, deployed, clip_sampler, mean, std, div255, short_side, crop_size, spatial_idx=(0, 1, 2),
                 frame_ratios=None, src_layout="NTHWC", method="sum", yuv=("bt709", False), coded_height=None, height=None):
        if getattr(deployed, "_pv_load_boxes", None) is not None:
            raise ValueError("VideoPredictor scores videos; a detection model's boxes belong to key frames"
                             " (in any source layout, %s included)" % src_layout)
        if method not in ("sum", "max"):
            raise NotImplementedError("ensemble method %r (the reference knows 'sum' and 'max')" % method)
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout,
                                   yuv, coded_height, height)
        self.sampler, self.method, self.src_layout = clip_sampler, method, src_layout
        self.video_ensembler = self.clip_ensembler = None

    @torch.no_grad()
    def __call__(self, video, fps, return_clip_scores=False):
        p = self.packer
        device = p.sess.device
        if video.dim() != (3 if p.is_yuv else 4):
            raise RuntimeError("expected one %d-d %s video, got %s" % (3 if p.is_yuv else 4, self.src_layout, tuple(video.shape)))
        num_frames = video.shape[1] if self.src_layout == "NCTHW" else video.shape[0]
        table, _ = clip_frame_table(self.sampler, num_frames, fps, p.clip_frames)
        tables = p.video_tables(table, num_frames)               # the one upload
        video = video.to(device, non_blocking=True)
        if not p.is_yuv:                                         # YUV frames are read in place, with the strides they have
            if video.dtype not in (torch.uint8, torch.float32):
                video = video.float()
            video = video.contiguous()
        n_clips, n_views, batch = table.shape[0], len(p.views), p.batch
        total = n_clips * n_views
        clip_of = torch.arange(total, dtype=torch.int32, device=device) // n_views
        zeros = torch.zeros(batch, dtype=torch.int32, device=device)
        for i0 in range(0, total, batch):
            n = min(batch, total - i0)
            p.fill_video(video, tables, i0, n)
            logits = p.launch()[:n]                              # rows of the zero-filled tail are never folded
            if i0 == 0:
                self.video_ensembler = VideoEnsembler(1, logits.shape[1], self.method, device)
                self.clip_ensembler = VideoEnsembler(n_clips, logits.shape[1], self.method, device) if return_clip_scores else None
            self.video_ensembler.update(logits, zeros[:n])
            if return_clip_scores:
                self.clip_ensembler.update(logits, clip_of[i0:i0 + n])
        scores = self.video_ensembler.result()[0]
        return (scores, self.clip_ensembler.result()) if return_clip_scores else scores
