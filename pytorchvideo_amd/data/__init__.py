"""The part of the reference's `pytorchvideo.data` that needs no decoder: the deterministic clip samplers and the frame
arithmetic that turns a sampler's clips into the frame table of the whole-video ingest (`pv_video_views`)."""
from .clip_sampling import (ClipInfo, ClipSampler, ConstantClipsPerVideoSampler, UniformClipSampler,  # noqa: F401
                            UniformClipSamplerTruncateFromStart, clip_frame_table, make_clip_sampler, sample_clips)
