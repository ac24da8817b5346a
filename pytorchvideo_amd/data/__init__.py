"""The part of the reference's `pytorchvideo.data` that needs no decoder: the deterministic clip samplers and the frame
arithmetic that turns a sampler's clips into the frame table of the whole-video ingest (`pv_video_views`), and the key-frame
windows of a detection run (`TimeStampClipSampler`, `keyframe_frame_table`), and the windows of a live stream as they complete (`stream_windows`)."""
from .clip_sampling import (ClipInfo, ClipSampler, ConstantClipsPerVideoSampler, TimeStampClipSampler,  # noqa: F401
                            UniformClipSampler, UniformClipSamplerTruncateFromStart, clip_frame_range, clip_frame_table,
                            keyframe_frame_table, make_clip_sampler, sample_clips, stream_windows)
