"""Whole-video inference: from one decoded video resident on the GPU to its scores, the reference's test protocol end to
end -- `LabeledVideoDataset` + clip sampler (data/clip_sampling.py), `FrameVideo.get_clip` (data/frame_video.py:149-200),
`UniformTemporalSubsample`, `ShortSideScale`, the three `uniform_crop`s, `Div255` + `Normalize`, the forward, and the
per-video fold of pytorchvideo_trainer/module/video_classification.py:244-311.

Nothing is materialised between the video and the first convolution: the sampler's clips become a table of frame numbers
on the host (`data.clip_frame_table`), the table is uploaded once, and the ingest kernel (`pv_video_views`) reads the video
through it, one launch per pathway per forward.  The clips x views sequence is walked in chunks of the deploy form's batch;
the last chunk may be short, so a video of any length runs on a form converted for any batch.

`VideoBatchPredictor` scores MANY videos per call -- a dataset evaluation -- with every forward filled by views of as many
videos as it takes (`pv_batch_views`: one source per item of the deploy batch), one table upload and at most one short chunk
per call instead of one of each per video.

`KeyframeDetector` is the same for the detection models: the reference's AVA recipe (the detection tutorial with
data/ava.py's `TimeStampClipSampler`) -- a clip around every key-frame time stamp, a variable number of person boxes per key
frame given in the pixels of the source frame -- with the boxes mapped into the view on the device (`pv_box_views`) and as many
key frames per forward as the deploy batch and the box capacity hold.

Every predictor also takes a video as a `transforms.FrameList` -- one device tensor per frame, as a hardware decoder's
surface pool hands them out -- and reads each frame where it lies (`pv_frame_views`); `StreamPredictor` scores a live
stream, whose frames arrive a few at a time, as its windows complete.
"""
import math
from fractions import Fraction

import torch

from .data.clip_sampling import clip_frame_table, keyframe_frame_table, stream_windows
from .ensemble import VideoEnsembler
from .transforms import (DevicePacker, FrameList, _interpolation, batch_chunks, box_regions, temporal_indices, track_boxes_at,
                         yuv_geometry)


def _resident(video, device, in_place):
    """The video on the device in a dtype the ingest reads: YUV frames and packed pixels (`DevicePacker.in_place`) are read in
    place, with the strides they have."""
    video = video.to(device, non_blocking=True)
    if in_place:
        return video
    if video.dtype not in (torch.uint8, torch.float32):
        video = video.float()
    return video.contiguous()


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
    `video` may also be a `transforms.FrameList` (one device tensor per frame): it is walked as a one-video batch
    (`packer.video_batch` / `fill_batch`, `pv_frame_views`), the same items at the same batch positions.
    `orientation` (`transforms.orientation_code`): the video is STORED turned and / or mirrored, as a decoder hands out a
    portrait phone clip; a non-zero code walks it as a one-video batch too and reads it in place.
    `hdr` ("pq", "hlg" or (transfer, `transforms.tone_params(...)`), for the 10- to 16-bit YUV layouts only): the video is
    BT.2020 PQ / HLG and every tap is mapped to BT.709 SDR inside the ingest launch (`pv_hdr_views`, as `DevicePacker`); such
    a predictor walks every video as a one-video batch.
    `interpolation="area"`: the short-side scale is the box filter of `transforms.short_side_scale(x, size, "area")` -- every
    source pixel under an output pixel averaged, what a 720p or larger source needs -- inside the ingest launch
    (`pv_area_views`, as `DevicePacker`); such a predictor walks every video as a one-video batch too.  A ValueError together
    with `hdr` or a non-zero `orientation`.
    After a call `video_ensembler.counts` (and `clip_ensembler.counts`) hold the rows folded."""

    def __init__(self, deployed, clip_sampler, mean, std, div255, short_side, crop_size, spatial_idx=(0, 1, 2),
                 frame_ratios=None, src_layout="NTHWC", method="sum", yuv=("bt709", False), coded_height=None, height=None,
                 hdr=None, interpolation="bilinear"):
        if getattr(deployed, "_pv_load_boxes", None) is not None:
            raise ValueError("VideoPredictor scores videos; a detection model's boxes belong to key frames"
                             " (in any source layout, %s included)" % src_layout)
        if method not in ("sum", "max"):
            raise NotImplementedError("ensemble method %r (the reference knows 'sum' and 'max')" % method)
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout,
                                   yuv, coded_height, height, hdr=hdr, interpolation=interpolation)
        self.sampler, self.method, self.src_layout = clip_sampler, method, src_layout
        self.video_ensembler = self.clip_ensembler = None

    @torch.no_grad()
    def __call__(self, video, fps, return_clip_scores=False, orientation=0):
        p = self.packer
        device = p.sess.device
        # HDR taps, the box filter and packed pixels: pv_hdr_views / pv_area_views / pv_batch_views, item-sourced launches
        if isinstance(video, FrameList) or orientation or p.hdr is not None or p.area or p.item_only:
            return self._call_frames(video, fps, return_clip_scores, orientation)
        if video.dim() != p.video_dims:
            raise RuntimeError("expected one %d-d %s video, got %s" % (p.video_dims, self.src_layout, tuple(video.shape)))
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

    def _call_frames(self, frames, fps, return_clip_scores, orientation=0):
        """A FrameList, or a video stored turned / mirrored (the one-source ingest has no orientation): the loop of `__call__`
        over a one-video batch."""
        p = self.packer
        device = p.sess.device
        if isinstance(frames, FrameList):
            num_frames = len(frames)
        else:
            if frames.dim() != p.video_dims:
                raise RuntimeError("expected one %d-d %s video, got %s" % (p.video_dims, self.src_layout, tuple(frames.shape)))
            num_frames = frames.shape[1] if self.src_layout == "NCTHW" else frames.shape[0]
            frames = _resident(frames, device, p.in_place)
        table, _ = clip_frame_table(self.sampler, num_frames, fps, p.clip_frames)
        batch = p.video_batch([frames], [table], orientation=orientation)    # every check, and the one upload
        zeros = torch.zeros(p.batch, dtype=torch.int32, device=device)
        for i0, n in batch_chunks(batch.total, p.batch):
            p.fill_batch(batch, i0, n)
            logits = p.launch()[:n]                              # rows of the zero-filled tail are never folded
            if i0 == 0:
                self.video_ensembler = VideoEnsembler(1, logits.shape[1], self.method, device)
                self.clip_ensembler = VideoEnsembler(batch.n_rows, logits.shape[1], self.method, device) if return_clip_scores else None
            self.video_ensembler.update(logits, zeros[:n])
            if return_clip_scores:
                self.clip_ensembler.update(logits, batch.clip_of[i0:i0 + n])
        p.release_batch()                                        # the frames are the caller's again
        scores = self.video_ensembler.result()[0]
        return (scores, self.clip_ensembler.result()) if return_clip_scores else scores


class VideoBatchPredictor:
    """`VideoBatchPredictor(deployed, clip_sampler, mean, std, div255, short_side, crop_size)(videos, fps)` = [V, num_classes]
    fp32 scores of a list of V videos, each folded as `VideoPredictor` folds one.  The videos are device tensors -- or ALL
    `transforms.FrameList`s, one device tensor per frame -- of ANY lengths and frame sizes in the one `src_layout` (for a
    YUV layout `height` / `coded_height` of the call are one number or one per video); `fps` is one number or one per video.  The views of all videos form one video-major sequence that is
    walked in chunks of the deploy batch, so a forward holds views of several videos and only the LAST forward of a call can
    be short; the frame tables of all videos are built, range-checked and uploaded once per call.
    `return_clip_scores=True` adds a list of V tensors [n_clips_j, num_classes].  `orientation` is one code
    (`transforms.orientation_code`) or one per video: videos stored turned and / or mirrored are read in place.  `hdr` as for
    `VideoPredictor`: one transfer and one tone table for the videos of the predictor.  `interpolation="area"` as for
    `VideoPredictor`: the box-filtered short-side scale (`pv_area_views`).  After a call
    `video_ensembler.counts` holds the views folded per video (and `clip_ensembler.counts` per clip, all videos' clips one after another)."""

    def __init__(self, deployed, clip_sampler, mean, std, div255, short_side, crop_size, spatial_idx=(0, 1, 2),
                 frame_ratios=None, src_layout="NTHWC", method="sum", yuv=("bt709", False), hdr=None,
                 interpolation="bilinear"):
        if getattr(deployed, "_pv_load_boxes", None) is not None:
            raise ValueError("VideoBatchPredictor scores videos; a detection model's boxes belong to key frames"
                             " (in any source layout, %s included)" % src_layout)
        if method not in ("sum", "max"):
            raise NotImplementedError("ensemble method %r (the reference knows 'sum' and 'max')" % method)
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout, yuv,
                                   hdr=hdr, interpolation=interpolation)
        self.sampler, self.method, self.src_layout = clip_sampler, method, src_layout
        self.video_ensembler = self.clip_ensembler = None
        self.forwards = 0                                        # forwards of the last call

    @torch.no_grad()
    def __call__(self, videos, fps, return_clip_scores=False, height=None, coded_height=None, orientation=None):
        p = self.packer
        device = p.sess.device
        videos = list(videos)
        if not videos:
            raise ValueError("no videos")
        rates = list(fps) if isinstance(fps, (list, tuple)) else [fps] * len(videos)
        if len(rates) != len(videos):
            raise ValueError("fps is one number or one per video: %d for %d videos" % (len(rates), len(videos)))
        dims = p.video_dims
        tables = []
        for j, (video, rate) in enumerate(zip(videos, rates)):
            if isinstance(video, FrameList):                     # its frames are checked by video_batch
                tables.append(clip_frame_table(self.sampler, len(video), rate, p.clip_frames)[0])
                continue
            if video.dim() != dims:
                raise RuntimeError("video %d: expected a %d-d %s video, got %s" % (j, dims, self.src_layout, tuple(video.shape)))
            num_frames = video.shape[1] if self.src_layout == "NCTHW" else video.shape[0]
            tables.append(clip_frame_table(self.sampler, num_frames, rate, p.clip_frames)[0])
        batch = p.video_batch(videos, tables, height, coded_height, orientation)    # every check, and the one upload
        self.forwards = 0
        for i0, n in batch_chunks(batch.total, p.batch):
            p.fill_batch(batch, i0, n)
            logits = p.launch()[:n]                              # rows of the zero-filled tail are never folded
            if i0 == 0:
                self.video_ensembler = VideoEnsembler(len(videos), logits.shape[1], self.method, device)
                self.clip_ensembler = VideoEnsembler(batch.n_rows, logits.shape[1], self.method, device) if return_clip_scores else None
            self.video_ensembler.update(logits, batch.video_of[i0:i0 + n])
            if return_clip_scores:
                self.clip_ensembler.update(logits, batch.clip_of[i0:i0 + n])
            self.forwards += 1
        p.release_batch()                                        # the videos are the caller's again
        scores = self.video_ensembler.result()
        if not return_clip_scores:
            return scores
        return scores, list(torch.split(self.clip_ensembler.result(), batch.clips))


def keyframe_chunks(counts, batch, capacity):
    """The forwards of a key-frame sequence whose key frame k has `counts[k]` boxes, for a deploy form of `batch` items
    and `capacity` box rows: a list of chunks, each the list of key-frame indices of one forward.  Key frames without a box
    are skipped (the tutorial skips them); the others are walked greedily in order -- a chunk takes key frames while it
    holds at most `batch` of them and at most `capacity` boxes, and a key frame is never split.  ValueError for a key frame
    with more than `capacity` boxes."""
    if batch < 1 or capacity < 1:
        raise ValueError("batch and capacity are positive")
    chunks, cur, used = [], [], 0
    for k, c in enumerate(int(c) for c in counts):
        if c < 0:
            raise ValueError("key frame %d has %d boxes" % (k, c))
        if c > capacity:
            raise ValueError("key frame %d has %d boxes, the deploy form was converted for at most %d" % (k, c, capacity))
        if c == 0:
            continue
        if cur and (len(cur) == batch or used + c > capacity):
            chunks.append(cur)
            cur, used = [], 0
        cur.append(k)
        used += c
    if cur:
        chunks.append(cur)
    return chunks


class KeyframeDetector:
    """`KeyframeDetector(deployed, clip_duration, mean, std, div255, short_side)(video, fps, timestamps, boxes)` =
    [sum r_k, num_classes] fp32 action scores, one row per person box, rows in the order of the concatenated box list.

    `deployed` is a detection model (`slow_r50_detection`, `slowfast_r50_detection`) converted as a whole by
    `convert_to_deployable_form(det, (x, bboxes))`: its batch is the number of key frames of one forward and its box count
    the CAPACITY of one forward.  `timestamps` are the key frames in seconds; around each a clip of `clip_duration` seconds is
    cut (`data.keyframe_frame_table`).  `boxes` holds one [r_k, 4] tensor (x1, y1, x2, y2 in the pixels of the SOURCE frame,
    finite; host or device) per time stamp, r_k >= 0; key frames without a box are skipped.  `crop_size=None` is the
    tutorial's protocol: boxes clipped to the frame, short side scaled to `short_side`, NO crop, boxes clipped again -- every
    video must then scale to the deploy form's H x W (256 x 455 for 720p at short_side 256).  With `crop_size` the view is the
    `spatial_idx` crop and the boxes follow it as `DevicePacker(dm)(clip, bboxes)` moves them.  `video`, `src_layout`, `yuv`,
    `coded_height`, `height` as for `VideoPredictor` (YUV 4:2:0 and `transforms.FrameList` included); `video` may also be a
    LIST of videos, with `timestamps` and `boxes` given per video and `fps` one number or one per video.  `orientation` is one
    code (`transforms.orientation_code`) or one per video: the video is stored turned and / or mirrored and the boxes are
    pixels of the STORED frame (a detector that ran on the decoder's surfaces); `pv_box_views` takes them into the view.
    `hdr` as for `VideoPredictor` (PQ / HLG sources in a 10- to 16-bit YUV layout, mapped to SDR per tap).
    `interpolation="area"` as for `VideoPredictor`: the box-filtered short-side scale (`pv_area_views`); the boxes depend on
    the geometry only and are mapped exactly as before.

    Frame tables, the box list and its key-frame index are uploaded once per call; per forward there are only the ingest,
    one `pv_box_views` launch and the replay.  The key frames are walked by `keyframe_chunks`.  Everything is validated
    before the first launch.  After a call `forwards` holds the number of forwards and `chunks` the key frames (numbered
    over all videos of the call, in order) of each."""

    def __init__(self, deployed, clip_duration, mean, std, div255, short_side, crop_size=None, spatial_idx=1,
                 frame_ratios=None, src_layout="NTHWC", yuv=("bt709", False), coded_height=None, height=None, hdr=None,
                 interpolation="bilinear"):
        if getattr(deployed, "_pv_load_boxes", None) is None or getattr(deployed, "_pv_box_capacity", None) is None:
            raise ValueError("KeyframeDetector scores the boxes of key frames with a detection model converted as a whole "
                             "by convert_to_deployable_form(det, (x, bboxes)); a classification model scores videos: "
                             "VideoPredictor / VideoBatchPredictor")
        if short_side is None:
            raise ValueError("short_side is required (crop_size=None: no crop)")
        if not isinstance(spatial_idx, int):
            raise ValueError("a detection model takes one view: its boxes belong to one crop")
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout,
                                   yuv, coded_height, height, keyframes=True, hdr=hdr, interpolation=interpolation)
        self.clip_duration, self.src_layout = clip_duration, src_layout
        self.forwards, self.chunks = 0, []

    @torch.no_grad()
    def __call__(self, video, fps, timestamps, boxes, height=None, coded_height=None, orientation=None):
        p = self.packer
        device = torch.device(p.sess.device)
        if isinstance(video, (list, tuple)):
            videos, stamps, box_lists = list(video), list(timestamps), list(boxes)
            rates = list(fps) if isinstance(fps, (list, tuple)) else [fps] * len(videos)
        else:
            videos, stamps, box_lists, rates = [video], [timestamps], [boxes], [fps]
        if not videos or not (len(stamps) == len(box_lists) == len(rates) == len(videos)):
            raise ValueError("timestamps, boxes and fps are given per video: %d, %d and %d for %d videos"
                             % (len(stamps), len(box_lists), len(rates), len(videos)))
        dims = p.video_dims

        def per_video(x):
            return list(x) if isinstance(x, (list, tuple)) else [x] * len(videos)

        heights, coded, orients = per_video(height), per_video(coded_height), per_video(orientation)
        if not (len(heights) == len(coded) == len(orients) == len(videos)):
            raise ValueError("height, coded_height and orientation are one value or one per video")
        kept, tables, counts, flat = [], [], [], []
        for j, (vid, rate, ts, bl) in enumerate(zip(videos, rates, stamps, box_lists)):
            as_frames = isinstance(vid, FrameList)               # its frames are checked by video_batch, and never moved
            if not as_frames and vid.dim() != dims:
                raise RuntimeError("video %d: expected a %d-d %s video, got %s" % (j, dims, self.src_layout, tuple(vid.shape)))
            ts, bl = list(ts), list(bl)
            if len(ts) != len(bl) or not ts:
                raise ValueError("video %d: %d box tensors for %d time stamps" % (j, len(bl), len(ts)))
            num_frames = len(vid) if as_frames else (vid.shape[1] if self.src_layout == "NCTHW" else vid.shape[0])
            table, _ = keyframe_frame_table(ts, self.clip_duration, num_frames, rate, p.clip_frames)
            for k, b in enumerate(bl):
                if not isinstance(b, torch.Tensor) or b.dim() != 2 or b.shape[1] != 4:
                    raise ValueError("video %d, key frame %d: boxes are an [r, 4] tensor (x1, y1, x2, y2)" % (j, k))
            own = [int(b.shape[0]) for b in bl]
            counts.extend(own)
            rows = [k for k, c in enumerate(own) if c > 0]
            if not rows:
                continue                                         # no key frame of this video has a box
            if not as_frames:
                vid = vid.to(device, non_blocking=True)
            if not as_frames and not p.in_place:
                if vid.dtype not in (torch.uint8, torch.float32):
                    vid = vid.float()
                vid = vid.contiguous()
            kept.append((vid, heights[j], coded[j], orients[j]))
            tables.append(table[rows])
            flat.extend(bl[k] for k in rows)
        chunks = keyframe_chunks(counts, p.batch, p.box_capacity)    # ValueError before any launch
        self.forwards, self.chunks = 0, chunks
        classes = p.model._pv_result().shape[1]
        out = torch.zeros((sum(counts), classes), dtype=torch.float32, device=device)
        if not chunks:
            return out
        batch = p.video_batch([k[0] for k in kept], tables, [k[1] for k in kept] if height is not None else None,
                              [k[2] for k in kept] if coded_height is not None else None,
                              [k[3] for k in kept] if orientation is not None else None)   # every check, one upload
        full = [c for c in counts if c > 0]                      # boxes per item of the sequence
        boxes_dev = torch.cat([b.detach().to(device=device, dtype=torch.float32) for b in flat]).contiguous()
        box_item = torch.repeat_interleave(torch.arange(len(full), dtype=torch.int32), torch.tensor(full)).to(device)
        item0 = box0 = 0
        for chunk in chunks:
            n_items = len(chunk)
            n = sum(counts[k] for k in chunk)
            p.fill_batch(batch, item0, n_items)
            p.fill_boxes(batch, boxes_dev, box_item, box0, n, item0, n_items)
            out[box0:box0 + n] = p.launch()[:n]                  # rows behind the n-th are padding
            item0, box0 = item0 + n_items, box0 + n
            self.forwards += 1
        p.release_batch()                                        # the videos are the caller's again
        return out


class TubePredictor:
    """`TubePredictor(deployed, clip_duration, mean, std, div255, crop_size)(video, fps, timestamps, boxes)` =
    [n_tubes, num_classes] fp32: the deploy form's output rows, one per ACTOR TUBE, in tube order (videos, then time stamps,
    then the boxes of a time stamp).  The commonest deployment of a classification model: a detector and a tracker find
    people, and the classifier is run on each person -- the person's rectangle of every frame of the clip, resized to the
    network's input.  Nothing is cropped, converted or resized in front of the ingest: the rectangles go to the device as a
    table, and the ingest reads each from the video where it lies (`pv_region_views`).

    `deployed` is a classification model converted as a whole by `convert_to_deployable_form`; `crop_size`, an int or
    (Ho, Wo), is its input size; `frame_ratios` as for `DevicePacker`.  Arguments are shaped as for `KeyframeDetector`:
    around each of `timestamps` (seconds) a clip of `clip_duration` seconds is cut (`data.keyframe_frame_table`), and
    `boxes[k]` is an [r_k, 4] tensor (x1, y1, x2, y2 in the pixels of the source frame, finite), r_k >= 0: r_k tubes, each
    static over the clip.  With `tracks` (then `boxes` is None) `tracks[k]` is a list of tubes, each a pair
    (frame_numbers [m], boxes [m, 4]) that is evaluated at the clip's frames (`transforms.track_boxes_at`): the rectangle
    moves with the actor.  A box becomes a rectangle by `transforms.box_regions(box, H, W, context, square, even)`, `even`
    for the YUV layouts.  `video` is one video, a list of videos (`timestamps`, `boxes` / `tracks` then per video, `fps`
    one number or one per video), or `transforms.FrameList`s; `src_layout`, `yuv`, `coded_height`, `height` as for
    `VideoPredictor`.

    Every tube is one item of the deploy batch; the tubes of all key frames and videos of a call fill the forwards
    (`batch_chunks`), so only the last one may be short.  Frame tables, rectangles and records are validated and uploaded
    once per call.  After a call `forwards` holds the number of forwards.  Stored-rotated videos and HDR sources are not
    taken here."""

    def __init__(self, deployed, clip_duration, mean, std, div255, crop_size, context=1.0, square=True, frame_ratios=None,
                 src_layout="NTHWC", yuv=("bt709", False), coded_height=None, height=None):
        if getattr(deployed, "_pv_load_boxes", None) is not None:
            raise ValueError("TubePredictor runs a classification model on every actor's own pixels; a detection model pools "
                             "its boxes from the whole frame's features: KeyframeDetector")
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, None, crop_size, 1, src_layout, yuv, coded_height,
                                   height, regions=True)
        self.clip_duration, self.src_layout = clip_duration, src_layout
        self.context, self.square = float(context), bool(square)
        self.forwards = 0

    @torch.no_grad()
    def __call__(self, video, fps, timestamps, boxes, tracks=None, height=None, coded_height=None):
        p = self.packer
        device = torch.device(p.sess.device)
        if (boxes is None) == (tracks is None):
            raise ValueError("give boxes (static over the clip) or tracks (a box per track point), one of them")
        tubes = boxes if tracks is None else tracks
        if isinstance(video, (list, tuple)):
            videos, stamps, tube_lists = list(video), list(timestamps), list(tubes)
            rates = list(fps) if isinstance(fps, (list, tuple)) else [fps] * len(videos)
        else:
            videos, stamps, tube_lists, rates = [video], [timestamps], [tubes], [fps]
        if not videos or not (len(stamps) == len(tube_lists) == len(rates) == len(videos)):
            raise ValueError("timestamps, boxes / tracks and fps are given per video: %d, %d and %d for %d videos"
                             % (len(stamps), len(tube_lists), len(rates), len(videos)))

        def per_video(x):
            return list(x) if isinstance(x, (list, tuple)) else [x] * len(videos)

        heights, coded = per_video(p.height if height is None else height), per_video(p.coded_height if coded_height is None else coded_height)
        if not (len(heights) == len(coded) == len(videos)):
            raise ValueError("height and coded_height are one value or one per video")
        dims = p.video_dims
        kept, tables, regions = [], [], []
        for j, (vid, rate, ts, tl) in enumerate(zip(videos, rates, stamps, tube_lists)):
            as_frames = isinstance(vid, FrameList)               # its frames are checked by video_batch, and never moved
            if not as_frames and vid.dim() != dims:
                raise RuntimeError("video %d: expected a %d-d %s video, got %s" % (j, dims, self.src_layout, tuple(vid.shape)))
            ts, tl = list(ts), list(tl)
            if len(ts) != len(tl) or not ts:
                raise ValueError("video %d: %d box / track entries for %d time stamps" % (j, len(tl), len(ts)))
            if as_frames:
                (_, hs, ws, _), num_frames = vid.geometry(self.src_layout, coded[j], heights[j]), len(vid)
            elif p.is_yuv:
                geom = yuv_geometry(vid, self.src_layout, coded[j], heights[j])
                hs, ws, num_frames = geom["Hs"], geom["Ws"], geom["N"]
            elif self.src_layout == "NCTHW":
                num_frames, hs, ws = vid.shape[1:]
            else:
                num_frames, hs, ws = vid.shape[:3]
            table, _ = keyframe_frame_table(ts, self.clip_duration, num_frames, rate, p.clip_frames)
            table = torch.as_tensor(table)
            rows, rects = [], []
            for k, entry in enumerate(tl):
                if tracks is None:
                    if not isinstance(entry, torch.Tensor) or entry.dim() != 2 or entry.shape[1] != 4:
                        raise ValueError("video %d, time stamp %d: boxes are an [r, 4] tensor (x1, y1, x2, y2)" % (j, k))
                    own = [r.expand(table.shape[1], 4) for r in box_regions(entry, hs, ws, self.context, self.square, even=p.region_even)]
                else:
                    own = [box_regions(track_boxes_at(fn, tb, table[k]), hs, ws, self.context, self.square, even=p.region_even)
                           for fn, tb in entry]
                rows.extend([k] * len(own))
                rects.extend(own)
            if not rows:
                continue                                         # no time stamp of this video has a tube
            if not as_frames:
                vid = _resident(vid, device, p.in_place)
            kept.append((vid, heights[j], coded[j]))
            tables.append(table[rows])
            regions.append(torch.stack(rects))
        self.forwards = 0
        classes = p.model._pv_result().shape[1]
        out = torch.zeros((sum(r.shape[0] for r in regions), classes), dtype=torch.float32, device=device)
        if not kept:
            return out
        batch = p.video_batch([k[0] for k in kept], tables, [k[1] for k in kept], [k[2] for k in kept],
                              regions=regions)                   # every check, and the one upload
        for i0, n in batch_chunks(batch.total, p.batch):
            p.fill_batch(batch, i0, n)
            out[i0:i0 + n] = p.launch()[:n]                      # rows of the zero-filled tail are padding
            self.forwards += 1
        p.release_batch()                                        # the videos are the caller's again
        return out


class StreamState:
    """The host bookkeeping of `StreamPredictor`, no device involved: which windows of a stream a push completes
    (`data.stream_windows`) and which frames may be dropped afterwards.  Absolute frame numbers are Python ints; `base` is
    the absolute number of the oldest frame still held and `next_window` the first window not yet emitted."""

    def __init__(self, clip_duration, stride, fps):
        self.duration, self.stride, self.fps = Fraction(clip_duration), Fraction(stride), Fraction(fps)
        if self.duration <= 0 or self.stride <= 0 or self.fps <= 0:
            raise ValueError("clip_duration, stride and fps are positive")
        self.seen = self.base = self.next_window = 0

    @property
    def held(self):
        return self.seen - self.base

    @property
    def bound(self):
        """`held` after a push of n frames is at most ceil(fps * clip_duration) + n: the first unemitted window is incomplete,
        so fewer than ceil(fps * d) + 1 of its frames had arrived before the push ended."""
        return math.ceil(self.fps * self.duration)

    def push(self, n):
        """`n` more frames have arrived: the windows (k, start_sec, first, stop) they complete, frames in ABSOLUTE numbers.
        The caller scores them -- every frame from `base` on is still held -- and then calls `drop()`."""
        if n < 0:
            raise ValueError("a push adds frames")
        self.seen += n
        windows = stream_windows(self.duration, self.stride, self.fps, self.seen, self.next_window)
        if windows:
            self.next_window = windows[-1][0] + 1
        return windows

    def drop(self):
        """Frames below the first frame of the first unemitted window are no longer needed: returns how many of the oldest
        held frames to let go, and moves `base` behind them."""
        keep_from = min(math.ceil(self.fps * (self.next_window * self.stride)), self.seen)
        n = max(0, keep_from - self.base)
        self.base += n
        return n


class StreamPredictor:
    """`StreamPredictor(deployed, clip_duration, stride, fps, mean, std, div255, short_side, crop_size).push(frames)` scores
    ONE live stream as its windows complete: window k covers [k * stride, k * stride + clip_duration) seconds of the stream
    (`data.stream_windows`: for a stream of at least one clip exactly the clips `UniformClipSampler(clip_duration, stride)`
    cuts from the frames seen so far), and `push` returns one (k, start_sec, scores) per window the pushed frames complete,
    `scores` a [num_classes] fp32 device tensor: the fold (`method`) over the window's views, the row `VideoPredictor`
    returns for that clip with `return_clip_scores=True`.

    `frames` is an iterable of per-frame device tensors in the forms of `transforms.FrameList` for `src_layout`; they are
    NOT copied -- the ingest reads each where it lies (`pv_frame_views`) -- and are held until no unemitted window needs
    them: after every push the frames in front of the first unemitted window are let go, so `frames_held` is at most
    ceil(fps * clip_duration) plus the size of the push.  The windows one push completes, times the views, are walked in
    chunks of the deploy batch from position 0; a short chunk zeroes the tail.  `push` enqueues its work on the launch stream
    and returns without waiting.  A decoder may therefore recycle a surface once the scores of the LAST window that contains
    it have been read on the host, or after a synchronise on the launch stream -- not when `push` returns.

    `orientation` (`transforms.orientation_code`): the frames are stored turned and / or mirrored and are read in place.
    `hdr` as for `VideoPredictor`: the surfaces are PQ / HLG and every tap is mapped to SDR inside the ingest launch.
    `interpolation="area"` as for `VideoPredictor`: the box-filtered short-side scale (`pv_area_views`).
    `deployed` is a classification form; one object scores one stream; `reset()` starts a new one.  Windows are scored
    independently: nothing is smoothed or voted over windows."""

    def __init__(self, deployed, clip_duration, stride, fps, mean, std, div255, short_side, crop_size, spatial_idx=(1,),
                 frame_ratios=None, src_layout="NTHWC", method="sum", yuv=("bt709", False), orientation=0, hdr=None,
                 interpolation="bilinear"):
        if getattr(deployed, "_pv_load_boxes", None) is not None:
            raise ValueError("StreamPredictor scores the windows of a stream with a classification form; a detection model's "
                             "boxes belong to key frames: KeyframeDetector")
        if method not in ("sum", "max"):
            raise NotImplementedError("ensemble method %r (the reference knows 'sum' and 'max')" % method)
        self.packer = DevicePacker(deployed, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout, yuv,
                                   hdr=hdr, interpolation=interpolation)
        _interpolation(interpolation, orientation, None, "StreamPredictor")   # a turned stream has no box filter: before any push
        self.method, self.src_layout, self.orientation = method, src_layout, orientation   # a stream has one orientation
        self.state = StreamState(clip_duration, stride, fps)
        self._frames = []
        self.forwards = 0                                        # forwards of the last push

    def reset(self):
        """Forget the stream: the next frame pushed is frame 0 of a new one."""
        self.state = StreamState(self.state.duration, self.state.stride, self.state.fps)
        self._frames = []

    @property
    def frames_held(self):
        return len(self._frames)

    @torch.no_grad()
    def push(self, frames):
        p = self.packer
        device = torch.device(p.sess.device)
        new = list(frames)
        self.forwards = 0
        if not new:
            return []
        held = FrameList(self._frames + new)                     # one form over the whole stream; refused before any change
        held.geometry(self.src_layout)
        if held.device.type != device.type or (device.index is not None and held.device.index != device.index):
            raise RuntimeError("the frames are on %s, the deploy form on %s" % (held.device, device))
        st = self.state
        base, batch = st.base, None
        windows = stream_windows(st.duration, st.stride, st.fps, st.seen + len(new), st.next_window)
        if windows:
            t = p.clip_frames
            table = torch.stack([first - base + temporal_indices(stop - first, t) for _, _, first, stop in windows]).to(torch.int32)
            batch = p.video_batch([held], [table], orientation=self.orientation)   # every check, the one upload: entries count from `base`
        self._frames = held.frames                               # nothing was refused: the push counts
        st.push(len(new))                                        # the same windows: stream_windows is pure
        out = []
        if windows:
            clips = None
            for i0, n in batch_chunks(batch.total, p.batch):
                p.fill_batch(batch, i0, n)
                logits = p.launch()[:n]                          # rows of the zero-filled tail are never folded
                if clips is None:
                    clips = VideoEnsembler(len(windows), logits.shape[1], self.method, device)
                clips.update(logits, batch.clip_of[i0:i0 + n])
                self.forwards += 1
            p.release_batch()
            scores = clips.result()
            out = [(k, start, scores[i]) for i, (k, start, _, _) in enumerate(windows)]
        del self._frames[:st.drop()]
        return out
