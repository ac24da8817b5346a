"""The deterministic clip samplers of the reference's data pipeline (pytorchvideo/data/clip_sampling.py) restated with the
same names, signatures and `Fraction` arithmetic, and `clip_frame_table`: the sampler's clips turned into the table of
frame numbers that `pv_video_views` (include/pv_mi355x.h) reads a video through -- the frame rule of
`FrameVideo.get_clip` (data/frame_video.py:149-200) followed by `UniformTemporalSubsample`.

Only the standard library is needed for the samplers; the random, training-time samplers are not restated
(`make_clip_sampler("random" | "random_multi")` raises NotImplementedError)."""
import math
from abc import ABC, abstractmethod
from fractions import Fraction
from typing import Any, Dict, List, NamedTuple, Optional, Tuple, Union


class ClipInfo(NamedTuple):
    """One sampled clip: [clip_start_sec, clip_end_sec) in seconds, its index in the video, the index of the augmentation
    (view) of that clip, and whether the video has no further clip."""
    clip_start_sec: Union[float, Fraction]
    clip_end_sec: Union[float, Fraction]
    clip_index: int
    aug_index: int
    is_last_clip: bool


class ClipSampler(ABC):
    """`sampler(last_clip_end_time, video_duration, annotation) -> ClipInfo`, called until `is_last_clip`."""

    def __init__(self, clip_duration: Union[float, Fraction]) -> None:
        self._clip_duration = Fraction(clip_duration)
        self._current_clip_index = 0
        self._current_aug_index = 0

    @abstractmethod
    def __call__(self, last_clip_end_time: Union[float, Fraction], video_duration: Union[float, Fraction],
                 annotation: Dict[str, Any]) -> ClipInfo:
        pass

    def reset(self) -> None:
        pass


class UniformClipSampler(ClipSampler):
    """Consecutive clips of `clip_duration`, `stride` apart (default: the clip duration).  `backpad_last` moves a last
    window that overhangs the end of the video back so that it ends with the video instead of dropping it."""

    def __init__(self, clip_duration: Union[float, Fraction], stride: Optional[Union[float, Fraction]] = None,
                 backpad_last: bool = False, eps: float = 1e-6):
        super().__init__(clip_duration)
        self._stride = self._clip_duration if stride is None else stride
        self._eps = eps
        self._backpad_last = backpad_last
        if not self._stride > 0:
            raise AssertionError("clips must advance: stride %r is not positive" % (stride,))

    def _clip_start_end(self, last_clip_end_time, video_duration, backpad_last) -> Tuple[Fraction, Fraction]:
        gap = self._stride - self._clip_duration          # from the end of one clip to the start of the next
        start = Fraction((-gap if last_clip_end_time is None else last_clip_end_time) + gap)
        end = Fraction(start + self._clip_duration)
        if backpad_last:
            start = Fraction(max(0, start - max(0, end - video_duration)))
            end = Fraction(start + self._clip_duration)
        return start, end

    def __call__(self, last_clip_end_time, video_duration, annotation) -> ClipInfo:
        start, end = self._clip_start_end(last_clip_end_time, video_duration, self._backpad_last)
        _, next_end = self._clip_start_end(end, video_duration, self._backpad_last)
        if self._backpad_last:                            # the next window would be this one again
            last = abs(next_end - end) < self._eps
        else:                                             # the next window overhangs the video
            last = (next_end - video_duration) > self._eps
        index = self._current_clip_index
        self._current_clip_index += 1
        if last:
            self.reset()
        return ClipInfo(start, end, index, 0, last)

    def reset(self):
        self._current_clip_index = 0


class UniformClipSamplerTruncateFromStart(UniformClipSampler):
    """UniformClipSampler over [0, min(truncation_duration, video_duration)]."""

    def __init__(self, clip_duration: Union[float, Fraction], stride: Optional[Union[float, Fraction]] = None,
                 backpad_last: bool = False, eps: float = 1e-6, truncation_duration: float = None) -> None:
        super().__init__(clip_duration, stride, backpad_last, eps)
        self.truncation_duration = truncation_duration

    def __call__(self, last_clip_end_time, video_duration, annotation) -> ClipInfo:
        if self.truncation_duration is not None:
            video_duration = min(self.truncation_duration, video_duration)
        return super().__call__(last_clip_end_time, video_duration, annotation)


class ConstantClipsPerVideoSampler(ClipSampler):
    """`clips_per_video` clips whose starts are evenly spaced over [0, video_duration - clip_duration], each returned
    `augs_per_clip` times with aug_index 0, 1, ... (the model zoo's "10 clips x 3 crops")."""

    def __init__(self, clip_duration: float, clips_per_video: int, augs_per_clip: int = 1) -> None:
        super().__init__(clip_duration)
        self._clips_per_video = clips_per_video
        self._augs_per_clip = augs_per_clip

    def __call__(self, last_clip_end_time, video_duration, annotation) -> ClipInfo:
        last_start = Fraction(max(video_duration - self._clip_duration, 0))
        step = Fraction(last_start, max(self._clips_per_video - 1, 1))
        index, aug = self._current_clip_index, self._current_aug_index
        start = step * index
        self._current_aug_index += 1
        if self._current_aug_index >= self._augs_per_clip:
            self._current_clip_index += 1
            self._current_aug_index = 0
        last = self._current_clip_index >= self._clips_per_video or step * self._current_clip_index > last_start
        if last:
            self.reset()
        return ClipInfo(start, start + self._clip_duration, index, aug, last)

    def reset(self):
        self._current_clip_index = 0
        self._current_aug_index = 0


class TimeStampClipSampler:
    """data/ava.py:282-318: the clip of `clip_sampler`'s duration CENTRED on the time stamp `annotation["clip_index"]` --
    [t - d/2, t - d/2 + d) -- for datasets such as AVA where only key frames are annotated.  clip_index, aug_index and
    is_last_clip are always 0, 0 and True.  As there, d is halved by the float 2.0, so the times are floats."""

    def __init__(self, clip_sampler: ClipSampler) -> None:
        self.clip_sampler = clip_sampler

    def __call__(self, last_clip_time, video_duration, annotation: Dict[str, Any]) -> ClipInfo:
        center_frame_sec = annotation["clip_index"]          # a.k.a. the time stamp
        clip_start_sec = center_frame_sec - self.clip_sampler._clip_duration / 2.0
        return ClipInfo(clip_start_sec, clip_start_sec + self.clip_sampler._clip_duration, 0, 0, True)

    def reset(self) -> None:
        pass


def make_clip_sampler(sampling_type: str, *args) -> ClipSampler:
    """"uniform" -> UniformClipSampler(*args); "constant_clips_per_video" -> ConstantClipsPerVideoSampler(*args)."""
    if sampling_type == "uniform":
        return UniformClipSampler(*args)
    if sampling_type == "constant_clips_per_video":
        return ConstantClipsPerVideoSampler(*args)
    if sampling_type in ("random", "random_multi"):
        raise NotImplementedError("the %r clip sampler is a training-time sampler; only the deterministic ones "
                                  "('uniform', 'constant_clips_per_video') are provided" % sampling_type)
    raise NotImplementedError("unknown clip sampler kind %r" % (sampling_type,))


def sample_clips(sampler: ClipSampler, video_duration) -> List[ClipInfo]:
    """Every ClipInfo the sampler yields for a video of `video_duration` seconds (the loop of LabeledVideoDataset)."""
    sampler.reset()
    clips, end = [], None
    while True:
        info = sampler(end, video_duration, {})
        clips.append(info)
        end = info.clip_end_sec
        if info.is_last_clip:
            return clips


def clip_frame_range(start_sec, end_sec, num_frames: int, fps: Fraction, what: str = "clip") -> Tuple[int, int]:
    """The frames range(first, stop) of an N-frame video that the clip [start_sec, end_sec) covers (frame_video.py:149-200):
    first = ceil(fps * start), stop = min(ceil(fps * min(end, duration)), N) with duration = N / fps -- a window that ends
    past the video is cut.  ValueError when the window starts before 0 or behind the video, or holds no frame."""
    duration = Fraction(num_frames) / fps
    start, end = Fraction(start_sec), min(Fraction(end_sec), duration)
    first = math.ceil(fps * start)
    stop = min(math.ceil(fps * end), num_frames)
    if start < 0 or start > duration or stop <= first:
        raise ValueError("%s [%s, %s) s holds no frame of a %d-frame video at %s fps" % (what, start_sec, end_sec, num_frames, fps))
    return first, stop


def clip_frame_table(sampler: ClipSampler, num_frames: int, fps, frames_per_clip: int):
    """(int32 [n_clips, frames_per_clip] tensor, [ClipInfo]): row i holds the frames of the video that clip i of `sampler`
    consists of.  A clip [start, end) covers frames range(ceil(fps * start), min(ceil(fps * min(end, duration)), N)) with
    duration = N / fps (frame_video.py:149-200), of which `transforms.temporal_indices` picks `frames_per_clip` (a video
    shorter than the clip repeats frames, as UniformTemporalSubsample does).  ClipInfos that differ only in aug_index --
    the views of one clip -- share a row; the returned list has one entry per row."""
    import torch
    from ..transforms import temporal_indices
    if num_frames <= 0 or frames_per_clip <= 0 or fps <= 0:
        raise ValueError("num_frames, fps and frames_per_clip are positive")
    fps = Fraction(fps)
    duration = Fraction(num_frames) / fps
    rows, infos = [], []
    for info in sample_clips(sampler, duration):
        if infos and info.clip_index == infos[-1].clip_index and info.aug_index != 0:
            continue
        first, stop = clip_frame_range(info.clip_start_sec, info.clip_end_sec, num_frames, fps, "clip %d" % info.clip_index)
        rows.append(first + temporal_indices(stop - first, frames_per_clip))
        infos.append(info)
    table = torch.stack(rows).to(torch.int32)
    if int(table.min()) < 0 or int(table.max()) >= num_frames:
        raise ValueError("frame table leaves the video [0, %d)" % num_frames)
    return table, infos


def keyframe_frame_table(timestamps, clip_duration, num_frames: int, fps, frames_per_clip: int):
    """(int32 [K, frames_per_clip] tensor, centre_frames [K]): row k holds the frames of the clip that `TimeStampClipSampler`
    cuts around key-frame time stamp `timestamps[k]` (seconds) -- the window [t - d/2, t - d/2 + d) of data/ava.py:310-315
    under the frame rule of `clip_frame_table` (a window that ends past the video is cut), the window computed in exact
    `Fraction` arithmetic on the numbers given (the sampler itself divides by the float 2.0, which can move a window edge
    that falls exactly on a frame by one frame) -- and `centre_frames[k]` the middle
    frame of that window, frames[len(frames) // 2]: the one the detection tutorial hands to the person detector
    (inp_imgs[:, shape[1] // 2]).  ValueError for a window that starts before 0 or holds no frame."""
    import torch
    from ..transforms import temporal_indices
    if num_frames <= 0 or frames_per_clip <= 0 or fps <= 0:
        raise ValueError("num_frames, fps and frames_per_clip are positive")
    stamps = list(timestamps)
    if not stamps:
        raise ValueError("no time stamps")
    fps = Fraction(fps)
    duration = Fraction(clip_duration)
    rows, centres = [], []
    for k, t in enumerate(stamps):
        start = Fraction(t) - duration / 2
        first, stop = clip_frame_range(start, start + duration, num_frames, fps, "key frame %d (t = %s s):" % (k, t))
        rows.append(first + temporal_indices(stop - first, frames_per_clip))
        centres.append(first + (stop - first) // 2)
    return torch.stack(rows).to(torch.int32), centres


def stream_windows(clip_duration, stride, fps, frames_seen: int, first_window: int = 0):
    """The windows of a live stream that are COMPLETE once `frames_seen` frames have arrived, from window `first_window`
    on: a list of (k, start_sec, first, stop).  Window k covers [k * stride, k * stride + clip_duration) seconds under the
    frame rule of `clip_frame_range` -- frames range(ceil(fps * start), ceil(fps * end)) -- in exact `Fraction` arithmetic,
    and is complete when its last frame has been seen: ceil(fps * end) <= frames_seen.  Its frame-table row is
    first + temporal_indices(stop - first, clip_frames).  A pure function of its arguments.

    For frames_seen / fps >= clip_duration these are exactly the clips `clip_frame_table(UniformClipSampler(clip_duration,
    stride), frames_seen, fps, T)` cuts from a video of `frames_seen` frames (for numbers that are exact fractions the
    sampler's eps never matters); a stream shorter than one clip has no complete window, where the sampler cuts one short
    clip."""
    d, step, fps = Fraction(clip_duration), Fraction(stride), Fraction(fps)
    if d <= 0 or step <= 0 or fps <= 0 or frames_seen < 0 or first_window < 0:
        raise ValueError("clip_duration, stride and fps are positive, frames_seen and first_window not negative")
    out, k = [], int(first_window)
    while True:
        start = k * step
        first, stop = math.ceil(fps * start), math.ceil(fps * (start + d))
        if stop > frames_seen:
            return out
        if stop <= first:
            raise ValueError("a window of %s s holds no frame at %s fps" % (d, fps))
        out.append((k, start, first, stop))
        k += 1
