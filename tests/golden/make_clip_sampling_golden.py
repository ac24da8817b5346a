"""Golden sequences for the clip samplers, produced by the REFERENCE'S OWN CODE (run where the
reference tree exists; the fixture travels, the reference does not).

pytorchvideo/data/clip_sampling.py imports only the standard library, so it is loaded by file path (importing the
`pytorchvideo.data` package would pull in the decoders).  Only OUTPUTS are recorded: for every case the constructor
arguments, the video duration and the `ClipInfo` sequence the sampler yields until `is_last_clip`, times as exact
numerator / denominator pairs.

    python tests/golden/make_clip_sampling_golden.py      # writes tests/golden/clip_sampling.json
"""
import importlib.util
import json
import os
import sys
from fractions import Fraction

REF = os.environ.get("PV_REFERENCE_ROOT", "/root/reference")
SRC = os.path.join(REF, "pytorchvideo", "data", "clip_sampling.py")


def enc(x):
    """A constructor argument or duration as JSON: ["F", num, den] for a Fraction, the value itself otherwise."""
    return ["F", x.numerator, x.denominator] if isinstance(x, Fraction) else x


def frac(x):
    x = Fraction(x)
    return [x.numerator, x.denominator]


def run(sampler, duration, limit=100000):
    out, end = [], None
    for _ in range(limit):
        c = sampler(end, duration, {})
        out.append([frac(c.clip_start_sec), frac(c.clip_end_sec), c.clip_index, c.aug_index, bool(c.is_last_clip)])
        end = c.clip_end_sec
        if c.is_last_clip:
            return out
    raise RuntimeError("sampler did not finish")


def cases():
    F = Fraction
    clip_f, clip_x = 2.0, F(32, 15)                       # a float and an exact clip duration
    durations = [0.7, 2.0, F(32, 15), F(1, 3), 10.0, F(300, 30), 61.3, F(1801, 30)]   # shorter, equal, much longer
    out = []
    for clip in (clip_f, clip_x):
        for dur in durations:
            for n in (1, 3, 10):
                for augs in (1, 3):
                    out.append(("ConstantClipsPerVideoSampler", [clip, n, augs], dur))
            for stride in (None, 0.5, F(16, 15)):
                for backpad in (False, True):
                    out.append(("UniformClipSampler", [clip, stride, backpad], dur))
            for trunc in (None, 1.0, 5.0):
                out.append(("UniformClipSamplerTruncateFromStart", [clip, None, False, 1e-6, trunc], dur))
                out.append(("UniformClipSamplerTruncateFromStart", [clip, F(1, 2), True, 1e-6, trunc], dur))
    # the docstring example of clip_sampling.py:122-131: 39 frames at 30 fps, clips of 32 frames, stride 16 frames
    for backpad in (False, True):
        out.append(("UniformClipSampler", [F(32, 30), F(16, 30), backpad], F(39, 30)))
    # the model zoo's protocol: 10 clips x 3 crops of a 10 s video, clips of 80 frames at 30 fps
    out.append(("ConstantClipsPerVideoSampler", [F(80, 30), 10, 3], F(300, 30)))
    return out


def main():
    spec = importlib.util.spec_from_file_location("ref_clip_sampling", SRC)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    recorded = []
    for name, args, dur in cases():
        sampler = getattr(ref, name)(*args)
        recorded.append({"sampler": name, "args": [enc(a) for a in args], "duration": enc(dur), "clips": run(sampler, dur)})
    made = ref.make_clip_sampler("constant_clips_per_video", 2.0, 5, 2)
    recorded.append({"sampler": "make_clip_sampler", "args": ["constant_clips_per_video", 2.0, 5, 2], "duration": 9.5,
                     "clips": run(made, 9.5)})
    made = ref.make_clip_sampler("uniform", 2.0)
    recorded.append({"sampler": "make_clip_sampler", "args": ["uniform", 2.0], "duration": 9.5, "clips": run(made, 9.5)})
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_sampling.json")
    with open(dst, "w") as f:
        json.dump({"source": os.path.relpath(SRC, REF), "cases": recorded}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", dst, len(recorded), "cases,", sum(len(c["clips"]) for c in recorded), "clips")


if __name__ == "__main__":
    sys.exit(main())
